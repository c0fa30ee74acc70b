/* Test-only driver: acm_index_matrix and acm_index_concat (acm_host.c, no HIP) under AddressSanitizer and UBSan,
 * and what acm_index runs on the host: acm_tally_batch's loop (acm_internal_cpu_tally_batch), then acm_index_matrix
 * (acm_index itself lives in the HIP translation unit, which this program does not link).  Every buffer is allocated at
 * its exact size, so that a byte read or written beside it is seen.  The machine's comparator is memcmp over 3-byte
 * symbols.  Built and run by tests/test_index_sanitized.py; exits 0 when every check held. */
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

int
main (void) {
  /* the worked example of include/acm_index.h: he, she, hers, s, qux over 14 texts; its count matrix by rows */
  const uint64_t n_texts = 14, n_keywords = 5, nnz = 17;
  uint64_t *row_ptr = exact ((uint64_t[]){ 0, 0, 1, 4, 7, 7, 7, 7, 10, 11, 12, 13, 17, 17, 17 }, 15 * sizeof (uint64_t));
  uint32_t *col = exact ((uint32_t[]){ 3, 0, 2, 3, 0, 1, 3, 0, 2, 3, 0, 3, 3, 0, 1, 2, 3 }, 17 * sizeof (uint32_t));
  uint64_t *val = exact ((uint64_t[]){ 1, 1, 1, 2, 1, 1, 3, 1, 1, 1, 1, 1, 1, 4, 2, 2, 4 }, 17 * sizeof (uint64_t));
  const uint64_t want_ptr[6] = { 0, 5, 7, 10, 17, 17 };
  const uint32_t want_text[17] = { 2, 3, 7, 8, 11, 3, 11, 2, 7, 11, 1, 2, 3, 7, 9, 10, 11 };
  const uint64_t want_count[17] = { 1, 1, 1, 1, 4, 1, 2, 1, 1, 2, 1, 2, 3, 1, 1, 1, 4 };
  uint64_t *post_ptr = room ((n_keywords + 1) * sizeof *post_ptr, 0xFF);
  uint32_t *post_text = room (nnz * sizeof *post_text, 0xFF);
  uint64_t *post_count = room (nnz * sizeof *post_count, 0xFF);
  uint64_t found = 99;
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, 0, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_OK);
  CHECK (found == nnz && memcmp (post_ptr, want_ptr, sizeof want_ptr) == 0 && memcmp (post_text, want_text, sizeof want_text) == 0 &&
         memcmp (post_count, want_count, sizeof want_count) == 0);
  /* the last text_base that fits, and one more */
  const uint64_t top_base = (1ull << 32) - n_texts;
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, top_base, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_OK);
  for (uint64_t e = 0; e < nnz; e++)
    CHECK (post_text[e] == (uint32_t)(top_base + want_text[e]));
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, top_base + 1, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_E_ARG);
  /* one entry too little room: the need, nothing written to the lists, post_ptr all the same; counting only; no text */
  uint32_t *small_text = room ((nnz - 1) * sizeof *small_text, '.');
  uint64_t *small_count = room ((nnz - 1) * sizeof *small_count, '.');
  memset (post_ptr, 0xFF, (n_keywords + 1) * sizeof *post_ptr);
  found = 99;
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, 0, post_ptr, small_text, small_count, nnz - 1, &found) == ACM_GPU_E_OVERFLOW);
  CHECK (found == nnz && memcmp (post_ptr, want_ptr, sizeof want_ptr) == 0 && all_bytes (small_text, (nnz - 1) * sizeof *small_text, '.') &&
         all_bytes (small_count, (nnz - 1) * sizeof *small_count, '.'));
  found = 99;
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, 0, post_ptr, NULL, NULL, 0, &found) == ACM_GPU_OK && found == nnz);
  uint64_t *zero = exact ((uint64_t[]){ 0 }, sizeof (uint64_t));
  CHECK (acm_index_matrix (zero, NULL, NULL, 0, n_keywords, 0, post_ptr, NULL, NULL, 0, &found) == ACM_GPU_OK && found == 0);
  for (uint64_t k = 0; k <= n_keywords; k++)
    CHECK (post_ptr[k] == 0);
  uint64_t *one_ptr = room (sizeof *one_ptr, 0x77); /* no keyword at all: one pointer */
  CHECK (acm_index_matrix (zero, NULL, NULL, 0, 0, 0, one_ptr, NULL, NULL, 0, &found) == ACM_GPU_OK && found == 0 && *one_ptr == 0);
  /* the refusals: a row_ptr that decreases or begins with 1, a col that is no keyword */
  row_ptr[2] = 5; /* (row_ptr[3] = 4) */
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, 0, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_E_ARG);
  row_ptr[2] = 1;
  row_ptr[0] = 1;
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, 0, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_E_ARG);
  row_ptr[0] = 0;
  col[16] = 5;
  CHECK (acm_index_matrix (row_ptr, col, val, n_texts, n_keywords, 0, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_E_ARG);
  col[16] = 3;
  /* CONCAT: texts 0 .. 6 over FOUR keywords (qux came later), texts 7 .. 13 at base 7 over five; every room exact */
  uint64_t *a_ptr = room (5 * sizeof *a_ptr, 0xFF), *b_ptr = room (6 * sizeof *b_ptr, 0xFF);
  uint32_t *a_text = room (7 * sizeof *a_text, 0xFF), *b_text = room (10 * sizeof *b_text, 0xFF);
  uint64_t *a_count = room (7 * sizeof *a_count, 0xFF), *b_count = room (10 * sizeof *b_count, 0xFF);
  uint64_t *b_rows = malloc (8 * sizeof *b_rows);
  CHECK (b_rows);
  for (int t = 0; t <= 7; t++)
    b_rows[t] = row_ptr[7 + t] - row_ptr[7];
  CHECK (acm_index_matrix (row_ptr, col, val, 7, 4, 0, a_ptr, a_text, a_count, 7, &found) == ACM_GPU_OK && found == 7);
  CHECK (acm_index_matrix (b_rows, col + 7, val + 7, 7, 5, 7, b_ptr, b_text, b_count, 10, &found) == ACM_GPU_OK && found == 10);
  memset (post_ptr, 0xFF, (n_keywords + 1) * sizeof *post_ptr);
  memset (post_text, 0xFF, nnz * sizeof *post_text);
  memset (post_count, 0xFF, nnz * sizeof *post_count);
  CHECK (acm_index_concat (a_ptr, a_text, a_count, 4, b_ptr, b_text, b_count, 5, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_OK);
  CHECK (found == nnz && memcmp (post_ptr, want_ptr, sizeof want_ptr) == 0 && memcmp (post_text, want_text, sizeof want_text) == 0 &&
         memcmp (post_count, want_count, sizeof want_count) == 0);
  memset (post_ptr, 0xFF, (n_keywords + 1) * sizeof *post_ptr);
  CHECK (acm_index_concat (a_ptr, a_text, a_count, 4, b_ptr, b_text, b_count, 5, post_ptr, small_text, small_count, nnz - 1, &found) ==
         ACM_GPU_E_OVERFLOW);
  CHECK (found == nnz && memcmp (post_ptr, want_ptr, sizeof want_ptr) == 0 && all_bytes (small_text, (nnz - 1) * sizeof *small_text, '.'));
  CHECK (acm_index_concat (a_ptr, a_text, a_count, 4, b_ptr, b_text, b_count, 5, post_ptr, NULL, NULL, 0, &found) == ACM_GPU_OK && found == nnz);
  /* the refusals: the wrong way round (a boundary, and more keywords in front), the same index twice, a pointer array that decreases */
  CHECK (acm_index_concat (b_ptr, b_text, b_count, 5, a_ptr, a_text, a_count, 4, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_E_ARG);
  CHECK (acm_index_concat (a_ptr, a_text, a_count, 4, a_ptr, a_text, a_count, 4, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_E_ARG);
  const uint64_t keep = b_ptr[2];
  b_ptr[2] = b_ptr[3] + 1;
  CHECK (acm_index_concat (a_ptr, a_text, a_count, 4, b_ptr, b_text, b_count, 5, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_E_ARG);
  b_ptr[2] = keep;
  /* what acm_index runs on the host: the loop and the count matrix, then the transposition, on 3-byte symbols */
  ACMachine *m = acm_create (cmp3, 0, 0);
  const char *words[5] = { "he", "she", "hers", "s", "qux" };
  unsigned char *letters[5];
  for (int k = 0; k < 5; k++) {
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
  const char *flat = "ushers and she sells sheon tophersxherssushers he she hers";
  uint64_t *off = exact ((uint64_t[]){ 0, 0, 2, 13, 24, 24, 30, 30, 34, 37, 39, 40, 58, 58, 58 }, 15 * sizeof (uint64_t));
  unsigned char *text = malloc (3 * 58);
  CHECK (text && strlen (flat) == 58);
  sym3 (text, flat, 58);
  uint64_t *m_ptr = room ((n_texts + 1) * sizeof *m_ptr, 0xFF);
  uint32_t *m_col = room (nnz * sizeof *m_col, 0xFF);
  uint64_t *m_val = room (nnz * sizeof *m_val, 0xFF);
  uint64_t total = 99;
  CHECK (acm_internal_cpu_tally_batch (m, text, off, n_texts, 3, m_ptr, m_col, m_val, nnz, &found, &total) == ACM_GPU_OK);
  CHECK (found == nnz && total == 28 && memcmp (m_ptr, row_ptr, 15 * sizeof *m_ptr) == 0 && memcmp (m_col, col, nnz * sizeof *m_col) == 0 &&
         memcmp (m_val, val, nnz * sizeof *m_val) == 0);
  memset (post_text, 0xFF, nnz * sizeof *post_text);
  CHECK (acm_index_matrix (m_ptr, m_col, m_val, n_texts, acm_nb_keywords (m), 0, post_ptr, post_text, post_count, nnz, &found) == ACM_GPU_OK);
  CHECK (memcmp (post_ptr, want_ptr, sizeof want_ptr) == 0 && memcmp (post_text, want_text, sizeof want_text) == 0 &&
         memcmp (post_count, want_count, sizeof want_count) == 0);
  free (m_val), free (m_col), free (m_ptr), free (text), free (off);
  acm_release (m);
  for (int k = 0; k < 5; k++)
    free (letters[k]);
  free (b_rows), free (b_count), free (a_count), free (b_text), free (a_text), free (b_ptr), free (a_ptr);
  free (one_ptr), free (zero), free (small_count), free (small_text), free (post_count), free (post_text), free (post_ptr);
  free (val), free (col), free (row_ptr);
  printf ("all checks held\n");
  return 0;
}
