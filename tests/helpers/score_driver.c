/* Test-only driver: acm_score_check, acm_score_matrix, acm_score_top and acm_score's host path (acm_host.c, no HIP)
 * under AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte read or written beside
 * it is seen; the sums of the wrapping matrix pass the ends of int64_t, which the host code must take in unsigned
 * arithmetic.  The machine's comparator is memcmp over 3-byte symbols, declared with acm_set_symbol_bytes: what acm_score
 * runs for it is the caller loop on the host, acm_internal_cpu_score (acm_score itself lives in the HIP translation unit,
 * which this program does not link).  Built and run by tests/test_score_sanitized.py; exits 0 when every check held. */
#include "aho_corasick.h"
#include "acm_gpu.h"
#include "acm_internal.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    if (!(x)) {                                                                                    \
      fprintf (stderr, "check failed: %s (%s:%d)\n", #x, __FILE__, __LINE__);                      \
      exit (1);                                                                                    \
    }                                                                                              \
  } while (0)

static void *
exact (const void *from, size_t bytes) {
  void *p = malloc (bytes ? bytes : 1);
  CHECK (p);
  if (bytes)
    memcpy (p, from, bytes);
  return p;
}

static void *
room (size_t bytes, int fill) {
  void *p = malloc (bytes ? bytes : 1);
  CHECK (p);
  memset (p, fill, bytes);
  return p;
}

static int
all_bytes (const void *p, size_t bytes, int fill) {
  for (size_t i = 0; i < bytes; i++)
    if (((const unsigned char *)p)[i] != (unsigned char)fill)
      return 0;
  return 1;
}

/* the letter c as a 3-byte symbol */
static void
sym3 (unsigned char *to, const char *word, size_t n) {
  for (size_t i = 0; i < n; i++) {
    to[3 * i] = (unsigned char)word[i];
    to[3 * i + 1] = (unsigned char)word[i] ^ 0x5A;
    to[3 * i + 2] = 7;
  }
}

static int
cmp3 (const void *a, const void *b, const void *arg) {
  (void)arg;
  return memcmp (a, b, 3);
}

#define NO_CAP ACM_SCORE_NO_CAP
#define NONE ACM_SCORE_NONE
#define BIG 2147483647

int
main (void) {
  /* the count matrix of {he, she, hers, s} (ids 0, 1, 2, 3) over the texts "", "us", "hers and sh", "e sells she", "",
   * "on top", "": us: s | hers and sh: he, hers, s x 2 | e sells she: he, she, s x 3 */
  const uint64_t n_texts = 7, n_classes = 7;
  uint64_t *row_ptr = exact ((uint64_t[]){ 0, 0, 1, 4, 7, 7, 7, 7 }, 8 * sizeof (uint64_t));
  uint32_t *col = exact ((uint32_t[]){ 3, 0, 2, 3, 0, 1, 3 }, 7 * sizeof (uint32_t));
  uint64_t *val = exact ((uint64_t[]){ 1, 1, 1, 2, 1, 1, 3 }, 7 * sizeof (uint64_t));
  /* the boundary model of include/acm_score.h without its class on qux: 0 a plain sum | 1 saturation | 2 an always-class
   * that he switches off | 3 one keyword twice | 4 cancelling, kept everywhere | 5 the extreme weights | 6 kept nowhere here */
  ACMScoreTerm *terms = exact ((ACMScoreTerm[]){ { 0, 3, NO_CAP }, { 2, 5, NO_CAP }, { 3, 2, 2 }, { 0, -4, NO_CAP }, { 3, 1, NO_CAP }, { 1, 1, 1 },
                                                 { 1, 10, NO_CAP }, { 0, 1, NO_CAP }, { 1, -1, NO_CAP }, { 2, -BIG - 1, NO_CAP }, { 3, BIG, 1 },
                                                 { 0, 3, NO_CAP }, { 3, 1, 3 } },
                               13 * sizeof (ACMScoreTerm));
  uint64_t *class_ptr = exact ((uint64_t[]){ 0, 2, 3, 5, 7, 9, 11, 13 }, 8 * sizeof (uint64_t));
  int64_t *bias = exact ((int64_t[]){ 0, 0, 2, 0, 0, -5, 0 }, 7 * sizeof (int64_t));
  int64_t *threshold = exact ((int64_t[]){ 1, 3, 1, 1, 0, -5, 7 }, 7 * sizeof (int64_t));
  CHECK (acm_score_check (terms, class_ptr, bias, threshold, n_classes, 4) == ACM_GPU_OK);
  CHECK (acm_score_check (terms, class_ptr, bias, threshold, n_classes, 3) == ACM_GPU_E_ARG); /* keyword 3 is none then */
  const uint64_t want_ptr[8] = { 0, 3, 6, 9, 15, 18, 21, 24 };
  const uint32_t want_class[24] = { 2, 4, 5, 2, 4, 5, 0, 1, 4, 0, 1, 2, 3, 4, 5, 2, 4, 5, 2, 4, 5, 2, 4, 5 };
  const int64_t far = 2147483642;
  const int64_t want_score[24] = { 2, 0, -5, 3, 0, far, 8, 4, 1, 3, 4, 1, 11, 0, far, 2, 0, -5, 2, 0, -5, 2, 0, -5 };
  const uint32_t want_best[7] = { 2, 5, 0, 5, 2, 2, 2 };
  uint64_t *kept_ptr = room ((n_texts + 1) * sizeof *kept_ptr, 0xFF);
  uint32_t *kept_class = room (24 * sizeof *kept_class, 0xFF);
  int64_t *kept_score = room (24 * sizeof *kept_score, 0xFF);
  uint32_t *best = room (n_texts * sizeof *best, 0xEE);
  uint64_t n_kept = 99;
  CHECK (acm_score_matrix (row_ptr, col, val, n_texts, 4, terms, class_ptr, bias, threshold, n_classes, kept_ptr, kept_class, kept_score, 24, &n_kept,
                           best) == ACM_GPU_OK);
  CHECK (n_kept == 24 && memcmp (kept_ptr, want_ptr, sizeof want_ptr) == 0 && memcmp (kept_class, want_class, sizeof want_class) == 0);
  CHECK (memcmp (kept_score, want_score, sizeof want_score) == 0 && memcmp (best, want_best, sizeof want_best) == 0);
  /* one entry too little room: the need, nothing written to the kept arrays or best, kept_ptr all the same */
  uint32_t *small_class = room (23 * sizeof *small_class, '.');
  int64_t *small_score = room (23 * sizeof *small_score, '.');
  memset (best, 0xEE, n_texts * sizeof *best);
  memset (kept_ptr, 0xFF, (n_texts + 1) * sizeof *kept_ptr);
  n_kept = 99;
  CHECK (acm_score_matrix (row_ptr, col, val, n_texts, 4, terms, class_ptr, bias, threshold, n_classes, kept_ptr, small_class, small_score, 23, &n_kept,
                           best) == ACM_GPU_E_OVERFLOW);
  CHECK (n_kept == 24 && memcmp (kept_ptr, want_ptr, sizeof want_ptr) == 0);
  CHECK (all_bytes (small_class, 23 * sizeof *small_class, '.') && all_bytes (small_score, 23 * sizeof *small_score, '.') &&
         all_bytes (best, n_texts * sizeof *best, 0xEE));
  /* counting only; no text at all; no class at all */
  n_kept = 99;
  CHECK (acm_score_matrix (row_ptr, col, val, n_texts, 4, terms, class_ptr, bias, threshold, n_classes, kept_ptr, NULL, NULL, 0, &n_kept, NULL) ==
           ACM_GPU_OK &&
         n_kept == 24);
  uint64_t *zero = exact ((uint64_t[]){ 0 }, sizeof (uint64_t));
  uint64_t *one_ptr = room (sizeof *one_ptr, 0x77);
  CHECK (acm_score_matrix (zero, NULL, NULL, 0, 4, terms, class_ptr, bias, threshold, n_classes, one_ptr, NULL, NULL, 0, &n_kept, NULL) == ACM_GPU_OK &&
         n_kept == 0 && *one_ptr == 0);
  CHECK (acm_score_matrix (row_ptr, col, val, n_texts, 4, NULL, zero, NULL, NULL, 0, kept_ptr, kept_class, kept_score, 24, &n_kept, best) == ACM_GPU_OK &&
         n_kept == 0);
  for (uint64_t t = 0; t <= n_texts; t++)
    CHECK (kept_ptr[t] == 0);
  for (uint64_t t = 0; t < n_texts; t++)
    CHECK (best[t] == NONE);
  /* TOP of the kept matrix above, k = 2: ties by text id, a column shorter than k, an empty column */
  memcpy (kept_ptr, want_ptr, sizeof want_ptr);
  memcpy (kept_class, want_class, sizeof want_class);
  memcpy (kept_score, want_score, sizeof want_score);
  uint64_t *hits = room (n_classes * sizeof *hits, 0xFF);
  uint32_t *top_n = room (n_classes * sizeof *top_n, 0xFF);
  uint32_t *top_text = room (n_classes * 2 * sizeof *top_text, 0xCC);
  int64_t *top_score = room (n_classes * 2 * sizeof *top_score, 0xCC);
  CHECK (acm_score_top (kept_ptr, kept_class, kept_score, n_texts, n_classes, 2, hits, top_n, top_text, top_score) == ACM_GPU_OK);
  const uint64_t want_hits[7] = { 2, 2, 6, 1, 7, 6, 0 };
  const uint32_t want_top_n[7] = { 2, 2, 2, 1, 2, 2, 0 };
  const uint32_t want_text[14] = { 2, 3, 2, 3, 1, 0, 3, NONE, 2, 0, 1, 3, NONE, NONE };
  const int64_t want_tscore[14] = { 8, 3, 4, 4, 3, 2, 11, 0, 1, 0, far, far, 0, 0 };
  CHECK (memcmp (hits, want_hits, sizeof want_hits) == 0 && memcmp (top_n, want_top_n, sizeof want_top_n) == 0);
  CHECK (memcmp (top_text, want_text, sizeof want_text) == 0 && memcmp (top_score, want_tscore, sizeof want_tscore) == 0);
  /* k = 0: the hits alone, no top arrays; k = 256 with exact rooms; the refusals */
  memset (hits, 0xFF, n_classes * sizeof *hits);
  CHECK (acm_score_top (kept_ptr, kept_class, kept_score, n_texts, n_classes, 0, hits, top_n, NULL, NULL) == ACM_GPU_OK);
  CHECK (memcmp (hits, want_hits, sizeof want_hits) == 0 && all_bytes (top_n, n_classes * sizeof *top_n, 0));
  uint32_t *wide_text = room (n_classes * 256 * sizeof *wide_text, 0xCC);
  int64_t *wide_score = room (n_classes * 256 * sizeof *wide_score, 0xCC);
  CHECK (acm_score_top (kept_ptr, kept_class, kept_score, n_texts, n_classes, 256, hits, top_n, wide_text, wide_score) == ACM_GPU_OK);
  CHECK (top_n[4] == 7 && wide_text[4 * 256 + 6] == 6 && wide_text[4 * 256 + 7] == NONE && wide_text[6 * 256 + 255] == NONE && wide_score[6 * 256 + 255] == 0);
  CHECK (acm_score_top (kept_ptr, kept_class, kept_score, n_texts, n_classes, 257, hits, top_n, wide_text, wide_score) == ACM_GPU_E_ARG);
  CHECK (acm_score_top (kept_ptr, kept_class, kept_score, n_texts, 5, 2, hits, top_n, top_text, top_score) == ACM_GPU_E_ARG); /* class 5 is kept */
  kept_ptr[2] = 10;
  CHECK (acm_score_top (kept_ptr, kept_class, kept_score, n_texts, n_classes, 2, hits, top_n, top_text, top_score) == ACM_GPU_E_ARG);
  kept_ptr[2] = 6;
  /* the wrapping matrix: counts of 2^40 and 2^63 under weights of +-(2^31 - 1); expected by hand, modulo 2^64 */
  uint64_t *w_ptr = exact ((uint64_t[]){ 0, 2, 2 }, 3 * sizeof (uint64_t));
  uint32_t *w_col = exact ((uint32_t[]){ 0, 1 }, 2 * sizeof (uint32_t));
  uint64_t *w_val = exact ((uint64_t[]){ 1ull << 40, 1ull << 63 }, 2 * sizeof (uint64_t));
  ACMScoreTerm *w_terms = exact ((ACMScoreTerm[]){ { 0, BIG, NO_CAP }, { 1, BIG, NO_CAP }, { 0, -BIG, NO_CAP }, { 1, -BIG, NO_CAP } }, 4 * sizeof (ACMScoreTerm));
  uint64_t *w_class_ptr = exact ((uint64_t[]){ 0, 2, 4 }, 3 * sizeof (uint64_t));
  int64_t *w_bias = exact ((int64_t[]){ 7, -1 }, 2 * sizeof (int64_t));
  int64_t *w_threshold = exact ((int64_t[]){ 8, INT64_MIN }, 2 * sizeof (int64_t));
  uint64_t *w_kept_ptr = room (3 * sizeof *w_kept_ptr, 0xFF);
  uint32_t *w_class = room (3 * sizeof *w_class, 0xFF), *w_best = room (2 * sizeof *w_best, 0xFF);
  int64_t *w_score = room (3 * sizeof *w_score, 0xFF);
  CHECK (acm_score_matrix (w_ptr, w_col, w_val, 2, 2, w_terms, w_class_ptr, w_bias, w_threshold, 2, w_kept_ptr, w_class, w_score, 3, &n_kept, w_best) ==
         ACM_GPU_OK);
  /* text 0: 7 - 2^40 + 2^63 and -1 + 2^40 + 2^63 (negative as a signed number); text 1: 7 is below 8, -1 is kept */
  CHECK (n_kept == 3 && w_kept_ptr[1] == 2 && w_kept_ptr[2] == 3 && w_class[0] == 0 && w_class[1] == 1 && w_class[2] == 1);
  CHECK (w_score[0] == 9223370937343148039ll && w_score[1] == -9223370937343148033ll && w_score[2] == -1 && w_best[0] == 0 && w_best[1] == 1);
  CHECK ((uint64_t)w_score[0] == 7ull + (uint64_t)BIG * (1ull << 40) + (uint64_t)BIG * (1ull << 63));
  uint64_t *w_hits = room (2 * sizeof *w_hits, 0xFF);
  uint32_t *w_top_n = room (2 * sizeof *w_top_n, 0xFF), *w_top_text = room (2 * sizeof *w_top_text, 0xFF);
  int64_t *w_top_score = room (2 * sizeof *w_top_score, 0xFF);
  CHECK (acm_score_top (w_kept_ptr, w_class, w_score, 2, 2, 1, w_hits, w_top_n, w_top_text, w_top_score) == ACM_GPU_OK);
  CHECK (w_hits[0] == 1 && w_hits[1] == 2 && w_top_text[0] == 0 && w_top_text[1] == 1 && w_top_score[1] == -1);
  /* the other refusals of the check */
  terms[2].cap = 0;
  CHECK (acm_score_check (terms, class_ptr, bias, threshold, n_classes, 4) == ACM_GPU_E_ARG);
  terms[2].cap = 2;
  class_ptr[1] = 4; /* (class_ptr[2] = 3) */
  CHECK (acm_score_check (terms, class_ptr, bias, threshold, n_classes, 4) == ACM_GPU_E_ARG);
  class_ptr[1] = 2;
  class_ptr[0] = 1;
  CHECK (acm_score_check (terms, class_ptr, bias, threshold, n_classes, 4) == ACM_GPU_E_ARG);
  class_ptr[0] = 0;
  CHECK (acm_score_check (terms, class_ptr, bias, threshold, 1ull << 31, 4) == ACM_GPU_E_ARG);
  CHECK (acm_score_check (terms, class_ptr, bias, threshold, n_classes, 4) == ACM_GPU_OK);
  row_ptr[2] = 5; /* (row_ptr[3] = 4) */
  CHECK (acm_score_matrix (row_ptr, col, val, n_texts, 4, terms, class_ptr, bias, threshold, n_classes, kept_ptr, kept_class, kept_score, 24, &n_kept,
                           best) == ACM_GPU_E_ARG);
  row_ptr[2] = 1;
  col[6] = 4;
  CHECK (acm_score_matrix (row_ptr, col, val, n_texts, 4, terms, class_ptr, bias, threshold, n_classes, kept_ptr, kept_class, kept_score, 24, &n_kept,
                           best) == ACM_GPU_E_ARG);
  col[6] = 3;
  /* what acm_score runs on the host: the loop, the count matrix in a room of the call's own, the evaluation and TOP above */
  ACMachine *m = acm_create (cmp3, 0, 0);
  const char *words[4] = { "he", "she", "hers", "s" };
  unsigned char *letters[4];
  for (int k = 0; k < 4; k++) {
    const size_t n = strlen (words[k]);
    letters[k] = malloc (3 * n);
    CHECK (letters[k]);
    sym3 (letters[k], words[k], n);
    const ACState *s = acm_initiate (m);
    for (size_t i = 0; i < n; i++)
      acm_insert_letter_of_keyword (&s, letters[k] + 3 * i);
    acm_insert_end_of_keyword (&s, 0, 0);
  }
  CHECK (acm_set_symbol_bytes (m, 3) == ACM_GPU_OK);
  const char *flat = "ushers and she sells sheon top";
  uint64_t *off = exact ((uint64_t[]){ 0, 0, 2, 13, 24, 24, 30, 30 }, 8 * sizeof (uint64_t));
  unsigned char *text = malloc (3 * 30);
  CHECK (text && strlen (flat) == 30);
  sym3 (text, flat, 30);
  uint64_t total = 99;
  n_kept = 99;
  memset (kept_ptr, 0xFF, (n_texts + 1) * sizeof *kept_ptr);
  memset (kept_class, 0xFF, 24 * sizeof *kept_class);
  memset (kept_score, 0xFF, 24 * sizeof *kept_score);
  memset (best, 0xEE, n_texts * sizeof *best);
  memset (top_text, 0xCC, n_classes * 2 * sizeof *top_text);
  CHECK (acm_internal_cpu_score (m, text, off, n_texts, 3, terms, class_ptr, bias, threshold, n_classes, kept_ptr, kept_class, kept_score, 24, &n_kept, best,
                                 2, hits, top_n, top_text, top_score, &total) == ACM_GPU_OK);
  CHECK (n_kept == 24 && total == 10 && memcmp (kept_ptr, want_ptr, sizeof want_ptr) == 0 && memcmp (kept_class, want_class, sizeof want_class) == 0);
  CHECK (memcmp (kept_score, want_score, sizeof want_score) == 0 && memcmp (best, want_best, sizeof want_best) == 0);
  CHECK (memcmp (hits, want_hits, sizeof want_hits) == 0 && memcmp (top_text, want_text, sizeof want_text) == 0 &&
         memcmp (top_score, want_tscore, sizeof want_tscore) == 0);
  memset (top_n, 0xAB, n_classes * sizeof *top_n);
  CHECK (acm_internal_cpu_score (m, text, off, n_texts, 3, terms, class_ptr, bias, threshold, n_classes, kept_ptr, small_class, small_score, 23, &n_kept,
                                 best, 2, hits, top_n, top_text, top_score, NULL) == ACM_GPU_E_OVERFLOW);
  CHECK (n_kept == 24 && memcmp (kept_ptr, want_ptr, sizeof want_ptr) == 0 && all_bytes (small_class, 23 * sizeof *small_class, '.') &&
         all_bytes (top_n, n_classes * sizeof *top_n, 0xAB));
  /* 1,500 texts "s he": 3,000 entries, more than the 1,024 the matrix room starts with, so it is grown */
  const uint64_t many = 1500;
  unsigned char *long_text = malloc (3 * 4 * many);
  uint64_t *long_off = malloc ((many + 1) * sizeof *long_off), *long_ptr = malloc ((many + 1) * sizeof *long_ptr);
  uint32_t *long_class = malloc (3 * many * sizeof *long_class), *long_best = malloc (many * sizeof *long_best);
  int64_t *long_score = malloc (3 * many * sizeof *long_score);
  CHECK (long_text && long_off && long_ptr && long_class && long_best && long_score);
  for (uint64_t t = 0; t < many; t++) {
    sym3 (long_text + 12 * t, "s he", 4);
    long_off[t] = 4 * t;
  }
  long_off[many] = 4 * many;
  /* he 1, s 1: class 0 scores 3, class 4 scores 1, class 5 scores 2^31 - 6; classes 1, 2 (2 - 4 + 1), 3 and 6 (4) stay out */
  CHECK (acm_internal_cpu_score (m, long_text, long_off, many, 3, terms, class_ptr, bias, threshold, n_classes, long_ptr, long_class, long_score, 3 * many,
                                 &n_kept, long_best, 0, NULL, NULL, NULL, NULL, &total) == ACM_GPU_OK);
  CHECK (n_kept == 3 * many && total == 2 * many && long_ptr[many] == 3 * many && long_class[3 * many - 1] == 5 && long_score[3 * many - 3] == 3 &&
         long_best[many - 1] == 5);
  free (long_score), free (long_best), free (long_class), free (long_ptr), free (long_off), free (long_text);
  free (text), free (off);
  acm_release (m);
  for (int k = 0; k < 4; k++)
    free (letters[k]);
  free (w_top_score), free (w_top_text), free (w_top_n), free (w_hits), free (w_score), free (w_best), free (w_class), free (w_kept_ptr);
  free (w_threshold), free (w_bias), free (w_class_ptr), free (w_terms), free (w_val), free (w_col), free (w_ptr);
  free (wide_score), free (wide_text), free (top_score), free (top_text), free (top_n), free (hits);
  free (one_ptr), free (zero), free (small_score), free (small_class), free (best), free (kept_score), free (kept_class), free (kept_ptr);
  free (threshold), free (bias), free (class_ptr), free (terms), free (val), free (col), free (row_ptr);
  printf ("all checks held\n");
  return 0;
}
