/* Test-only driver: acm_cooccur_matrix and acm_cooccur_add (acm_host.c, no HIP) under AddressSanitizer and UBSan,
 * and what acm_cooccur runs on the host: acm_tally_batch's loop (acm_internal_cpu_tally_batch), then acm_cooccur_matrix
 * (acm_cooccur itself lives in the HIP translation unit, which this program does not link).  Every buffer is allocated at
 * its exact size, so that a byte read or written beside it is seen.  The machine's comparator is memcmp over 3-byte
 * symbols.  Built and run by tests/test_cooccur_sanitized.py; exits 0 when every check held. */
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

/* the tables of include/acm_cooccur.h by flags: 0, PRODUCT, DIAGONAL, PRODUCT | DIAGONAL */
static const uint64_t want_ptr[2][6] = { { 0, 3, 5, 6, 6, 6 }, { 0, 4, 7, 9, 10, 10 } };
static const uint32_t want_col[2][10] = { { 1, 2, 3, 2, 3, 3 }, { 0, 1, 2, 3, 1, 2, 3, 2, 3, 3 } };
static const uint64_t want_val[4][10] = { { 2, 3, 4, 1, 2, 3 },
                                          { 9, 10, 22, 4, 11, 11 },
                                          { 5, 2, 3, 4, 2, 1, 2, 3, 3, 7 },
                                          { 20, 9, 10, 22, 5, 4, 11, 6, 11, 33 } };
static const uint64_t want_nnz[2] = { 6, 10 }, want_cross[2] = { 15, 32 };

int
main (void) {
  /* the worked example: he, she, hers, s, qux over 14 texts; its count matrix by rows */
  const uint64_t n_texts = 14, n_keywords = 5, entries = 17;
  uint64_t *row_ptr = exact ((uint64_t[]){ 0, 0, 1, 4, 7, 7, 7, 7, 10, 11, 12, 13, 17, 17, 17 }, 15 * sizeof (uint64_t));
  uint32_t *col = exact ((uint32_t[]){ 3, 0, 2, 3, 0, 1, 3, 0, 2, 3, 0, 3, 3, 0, 1, 2, 3 }, 17 * sizeof (uint32_t));
  uint64_t *val = exact ((uint64_t[]){ 1, 1, 1, 2, 1, 1, 3, 1, 1, 1, 1, 1, 1, 4, 2, 2, 4 }, 17 * sizeof (uint64_t));
  uint64_t *b_rows = malloc (8 * sizeof *b_rows); /* texts 7 .. 13 as a matrix of their own */
  CHECK (b_rows);
  for (int t = 0; t <= 7; t++)
    b_rows[t] = row_ptr[7 + t] - row_ptr[7];
  uint64_t found = 99, cross = 99, skipped = 99;
  for (uint32_t flags = 0; flags < 4; flags++) {
    const int d = (flags & ACM_COOCCUR_DIAGONAL) != 0;
    const uint64_t nnz = want_nnz[d];
    uint64_t *co_ptr = room ((n_keywords + 1) * sizeof *co_ptr, 0xFF);
    uint32_t *co_col = room (nnz * sizeof *co_col, 0xFF);
    uint64_t *co_val = room (nnz * sizeof *co_val, 0xFF);
    CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, flags, 0, co_ptr, co_col, co_val, nnz, &found, &cross, &skipped) == ACM_GPU_OK);
    CHECK (found == nnz && cross == want_cross[d] && skipped == 0 && memcmp (co_ptr, want_ptr[d], sizeof want_ptr[d]) == 0 &&
           memcmp (co_col, want_col[d], nnz * sizeof *co_col) == 0 && memcmp (co_val, want_val[flags], nnz * sizeof *co_val) == 0);
    /* one entry too little room: the need, nothing written to the entries, co_ptr all the same; counting only */
    uint32_t *small_col = room ((nnz - 1) * sizeof *small_col, '.');
    uint64_t *small_val = room ((nnz - 1) * sizeof *small_val, '.');
    memset (co_ptr, 0xFF, (n_keywords + 1) * sizeof *co_ptr);
    found = cross = 99;
    CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, flags, 0, co_ptr, small_col, small_val, nnz - 1, &found, &cross, &skipped) ==
           ACM_GPU_E_OVERFLOW);
    CHECK (found == nnz && cross == want_cross[d] && memcmp (co_ptr, want_ptr[d], sizeof want_ptr[d]) == 0 &&
           all_bytes (small_col, (nnz - 1) * sizeof *small_col, '.') && all_bytes (small_val, (nnz - 1) * sizeof *small_val, '.'));
    found = 99;
    CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, flags, 0, co_ptr, NULL, NULL, 0, &found, NULL, NULL) == ACM_GPU_OK && found == nnz);
    /* ADD: texts 0 .. 6 over FOUR keywords (qux came later) plus texts 7 .. 13 over five; every room exact */
    uint64_t *a_ptr = room (5 * sizeof *a_ptr, 0xFF), *b_ptr = room (6 * sizeof *b_ptr, 0xFF);
    uint64_t na = 99, nb = 99;
    CHECK (acm_cooccur_matrix (row_ptr, col, val, 7, 4, flags, 0, a_ptr, NULL, NULL, 0, &na, NULL, NULL) == ACM_GPU_OK && na > 0);
    CHECK (acm_cooccur_matrix (b_rows, col + 7, val + 7, 7, 5, flags, 0, b_ptr, NULL, NULL, 0, &nb, NULL, NULL) == ACM_GPU_OK && nb == nnz);
    uint32_t *a_col = room (na * sizeof *a_col, 0xFF), *b_col = room (nb * sizeof *b_col, 0xFF);
    uint64_t *a_val = room (na * sizeof *a_val, 0xFF), *b_val = room (nb * sizeof *b_val, 0xFF);
    CHECK (acm_cooccur_matrix (row_ptr, col, val, 7, 4, flags, 0, a_ptr, a_col, a_val, na, &found, &cross, &skipped) == ACM_GPU_OK && found == na);
    CHECK (acm_cooccur_matrix (b_rows, col + 7, val + 7, 7, 5, flags, 0, b_ptr, b_col, b_val, nb, &found, &cross, &skipped) == ACM_GPU_OK && found == nb);
    memset (co_ptr, 0xFF, (n_keywords + 1) * sizeof *co_ptr);
    memset (co_col, 0xFF, nnz * sizeof *co_col);
    memset (co_val, 0xFF, nnz * sizeof *co_val);
    CHECK (acm_cooccur_add (a_ptr, a_col, a_val, 4, b_ptr, b_col, b_val, 5, co_ptr, co_col, co_val, nnz, &found) == ACM_GPU_OK);
    CHECK (found == nnz && memcmp (co_ptr, want_ptr[d], sizeof want_ptr[d]) == 0 && memcmp (co_col, want_col[d], nnz * sizeof *co_col) == 0 &&
           memcmp (co_val, want_val[flags], nnz * sizeof *co_val) == 0);
    memset (co_ptr, 0xFF, (n_keywords + 1) * sizeof *co_ptr);
    CHECK (acm_cooccur_add (a_ptr, a_col, a_val, 4, b_ptr, b_col, b_val, 5, co_ptr, small_col, small_val, nnz - 1, &found) == ACM_GPU_E_OVERFLOW);
    CHECK (found == nnz && memcmp (co_ptr, want_ptr[d], sizeof want_ptr[d]) == 0 && all_bytes (small_col, (nnz - 1) * sizeof *small_col, '.'));
    CHECK (acm_cooccur_add (a_ptr, a_col, a_val, 4, b_ptr, b_col, b_val, 5, co_ptr, NULL, NULL, 0, &found) == ACM_GPU_OK && found == nnz);
    /* the refusals: more keywords in front, a pointer array that decreases, a col that is no keyword */
    CHECK (acm_cooccur_add (b_ptr, b_col, b_val, 5, a_ptr, a_col, a_val, 4, co_ptr, co_col, co_val, nnz, &found) == ACM_GPU_E_ARG);
    const uint64_t keep = b_ptr[2];
    b_ptr[2] = b_ptr[3] + 1;
    CHECK (acm_cooccur_add (a_ptr, a_col, a_val, 4, b_ptr, b_col, b_val, 5, co_ptr, co_col, co_val, nnz, &found) == ACM_GPU_E_ARG);
    b_ptr[2] = keep;
    b_col[nb - 1] = 5;
    CHECK (acm_cooccur_add (a_ptr, a_col, a_val, 4, b_ptr, b_col, b_val, 5, co_ptr, co_col, co_val, nnz, &found) == ACM_GPU_E_ARG);
    free (b_val), free (a_val), free (b_col), free (a_col), free (b_ptr), free (a_ptr);
    free (small_val), free (small_col), free (co_val), free (co_col), free (co_ptr);
  }
  /* row_limit = 3: text 11 is skipped */
  uint64_t *co_ptr = room ((n_keywords + 1) * sizeof *co_ptr, 0xFF);
  uint32_t *co_col = room (5 * sizeof *co_col, 0xFF);
  uint64_t *co_val = room (5 * sizeof *co_val, 0xFF);
  CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, 0, 3, co_ptr, co_col, co_val, 5, &found, &cross, &skipped) == ACM_GPU_OK);
  CHECK (found == 5 && cross == 9 && skipped == 1 && memcmp (co_col, (uint32_t[]){ 1, 2, 3, 3, 3 }, 5 * sizeof *co_col) == 0 &&
         memcmp (co_val, (uint64_t[]){ 1, 2, 3, 1, 2 }, 5 * sizeof *co_val) == 0);
  /* no text; no keyword at all: one pointer */
  uint64_t *zero = exact ((uint64_t[]){ 0 }, sizeof (uint64_t));
  CHECK (acm_cooccur_matrix (zero, NULL, NULL, 0, n_keywords, 3, 0, co_ptr, NULL, NULL, 0, &found, &cross, &skipped) == ACM_GPU_OK);
  CHECK (found == 0 && cross == 0 && skipped == 0);
  for (uint64_t k = 0; k <= n_keywords; k++)
    CHECK (co_ptr[k] == 0);
  uint64_t *one_ptr = room (sizeof *one_ptr, 0x77);
  CHECK (acm_cooccur_matrix (zero, NULL, NULL, 0, 0, 0, 0, one_ptr, NULL, NULL, 0, &found, NULL, NULL) == ACM_GPU_OK && found == 0 && *one_ptr == 0);
  CHECK (acm_cooccur_add (zero, NULL, NULL, 0, zero, NULL, NULL, 0, one_ptr, NULL, NULL, 0, &found) == ACM_GPU_OK && found == 0 && *one_ptr == 0);
  /* the refusals: a row_ptr that decreases or begins with 1, a col that is no keyword, a row that repeats one, a flag bit */
  row_ptr[2] = 5; /* (row_ptr[3] = 4) */
  CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, 0, 0, co_ptr, co_col, co_val, 5, &found, &cross, &skipped) == ACM_GPU_E_ARG);
  row_ptr[2] = 1;
  row_ptr[0] = 1;
  CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, 0, 0, co_ptr, co_col, co_val, 5, &found, &cross, &skipped) == ACM_GPU_E_ARG);
  row_ptr[0] = 0;
  col[16] = 5;
  CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, 0, 0, co_ptr, co_col, co_val, 5, &found, &cross, &skipped) == ACM_GPU_E_ARG);
  col[16] = 2;
  CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, 0, 0, co_ptr, co_col, co_val, 5, &found, &cross, &skipped) == ACM_GPU_E_ARG);
  col[16] = 3;
  CHECK (acm_cooccur_matrix (row_ptr, col, val, n_texts, n_keywords, 4, 0, co_ptr, co_col, co_val, 5, &found, &cross, &skipped) == ACM_GPU_E_ARG);
  /* products that wrap: (2^64 - 1)^2 = 1, 2^32 * 2^32 = 0 (the entry stays) */
  uint64_t *w_ptr = exact ((uint64_t[]){ 0, 2, 4 }, 3 * sizeof (uint64_t));
  uint32_t *w_col = exact ((uint32_t[]){ 0, 1, 0, 1 }, 4 * sizeof (uint32_t));
  uint64_t *w_val = exact ((uint64_t[]){ UINT64_MAX, UINT64_MAX, 1ull << 32, 1ull << 32 }, 4 * sizeof (uint64_t));
  CHECK (acm_cooccur_matrix (w_ptr, w_col, w_val, 2, 2, ACM_COOCCUR_PRODUCT, 0, co_ptr, co_col, co_val, 1, &found, &cross, &skipped) == ACM_GPU_OK);
  CHECK (found == 1 && cross == 2 && co_col[0] == 1 && co_val[0] == 1);
  /* what acm_cooccur runs on the host: the loop and the count matrix, then the definition, on 3-byte symbols */
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
  uint32_t *m_col = room (entries * sizeof *m_col, 0xFF);
  uint64_t *m_val = room (entries * sizeof *m_val, 0xFF);
  uint64_t total = 99;
  CHECK (acm_internal_cpu_tally_batch (m, text, off, n_texts, 3, m_ptr, m_col, m_val, entries, &found, &total) == ACM_GPU_OK);
  CHECK (found == entries && total == 28 && memcmp (m_ptr, row_ptr, 15 * sizeof *m_ptr) == 0 && memcmp (m_col, col, entries * sizeof *m_col) == 0 &&
         memcmp (m_val, val, entries * sizeof *m_val) == 0);
  uint32_t *d_col = room (10 * sizeof *d_col, 0xFF);
  uint64_t *d_val = room (10 * sizeof *d_val, 0xFF);
  CHECK (acm_cooccur_matrix (m_ptr, m_col, m_val, n_texts, acm_nb_keywords (m), 3, 0, co_ptr, d_col, d_val, 10, &found, &cross, &skipped) == ACM_GPU_OK);
  CHECK (found == 10 && cross == 32 && memcmp (co_ptr, want_ptr[1], sizeof want_ptr[1]) == 0 && memcmp (d_col, want_col[1], 10 * sizeof *d_col) == 0 &&
         memcmp (d_val, want_val[3], 10 * sizeof *d_val) == 0);
  free (d_val), free (d_col), free (m_val), free (m_col), free (m_ptr), free (text), free (off);
  acm_release (m);
  for (int k = 0; k < 5; k++)
    free (letters[k]);
  free (w_val), free (w_col), free (w_ptr), free (one_ptr), free (zero), free (co_val), free (co_col), free (co_ptr);
  free (b_rows), free (val), free (col), free (row_ptr);
  printf ("all checks held\n");
  return 0;
}
