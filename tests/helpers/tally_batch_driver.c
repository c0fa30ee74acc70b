/* Test-only driver: acm_tally_batch_records and acm_tally_batch's host path (acm_host.c, no HIP)
 * under AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte
 * read or written beside it is seen.  The machine's comparator is memcmp over 3-byte symbols,
 * declared with acm_set_symbol_bytes: what acm_tally_batch runs for it is the caller loop on the
 * host.  The loop and the sequential pass are called on their own, and then
 * acm_internal_cpu_tally_batch, the very function acm_tally_batch calls for such a machine
 * (acm_tally_batch itself lives in the HIP translation unit, which this program does not link).
 * Built and run by tests/test_tally_batch_sanitized.py; exits 0 when every check held. */
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
  /* {he, she, hers, s} (ids 0, 1, 2, 3) over the texts "", "us", "hers and sh", "e sells she", "", "on top", "":
   * "us|hers" and "sh|e" cut a keyword, "on top" has no match, the empty texts sit at the front, in the middle
   * and at the end */
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
  const uint64_t cuts[8] = { 0, 0, 2, 13, 24, 24, 30, 30 };
  const uint64_t n_texts = 7, n_sym = 30;
  CHECK (strlen (flat) == n_sym);
  unsigned char *text = malloc (3 * n_sym);
  CHECK (text);
  sym3 (text, flat, n_sym);
  uint64_t *off = exact (cuts, sizeof cuts);
  /* the caller loop into a room of exactly the 10 records; one less is an overflow that says so */
  ACMRecord *records = malloc (10 * sizeof *records);
  uint64_t *first = malloc ((n_texts + 1) * sizeof *first);
  CHECK (records && first);
  uint64_t found = 0;
  CHECK (acm_internal_cpu_scan_batch (m, text, off, n_texts, 3, records, NULL, first, 9, &found) == ACM_GPU_E_OVERFLOW && found == 10);
  CHECK (acm_internal_cpu_scan_batch (m, text, off, n_texts, 3, records, NULL, first, 10, &found) == ACM_GPU_OK && found == 10);
  /* us: s | hers and sh: he, hers, s, s | e sells she: s, s, s, she, he | on top: none */
  const uint64_t want_ptr[8] = { 0, 0, 1, 4, 7, 7, 7, 7 };
  const uint32_t want_col[7] = { 3, 0, 2, 3, 0, 1, 3 };
  const uint64_t want_val[7] = { 1, 1, 1, 2, 1, 1, 3 };
  uint64_t *row_ptr = malloc ((n_texts + 1) * sizeof *row_ptr);
  uint32_t *col = malloc (7 * sizeof *col);
  uint64_t *val = malloc (7 * sizeof *val);
  CHECK (row_ptr && col && val);
  uint64_t nnz = 99;
  CHECK (acm_tally_batch_records (records, first, n_texts, acm_nb_keywords (m), row_ptr, col, val, 7, &nnz) == ACM_GPU_OK);
  CHECK (nnz == 7 && memcmp (row_ptr, want_ptr, sizeof want_ptr) == 0);
  CHECK (memcmp (col, want_col, sizeof want_col) == 0 && memcmp (val, want_val, sizeof want_val) == 0);
  /* one entry too little room: the need, nothing written to col and val, row_ptr all the same */
  uint32_t *small_col = malloc (6 * sizeof *small_col);
  uint64_t *small_val = malloc (6 * sizeof *small_val);
  CHECK (small_col && small_val);
  memset (small_col, '.', 6 * sizeof *small_col);
  memset (small_val, '.', 6 * sizeof *small_val);
  memset (row_ptr, 0xFF, (n_texts + 1) * sizeof *row_ptr);
  nnz = 99;
  CHECK (acm_tally_batch_records (records, first, n_texts, 4, row_ptr, small_col, small_val, 6, &nnz) == ACM_GPU_E_OVERFLOW);
  CHECK (nnz == 7 && memcmp (row_ptr, want_ptr, sizeof want_ptr) == 0);
  for (size_t i = 0; i < 6 * sizeof *small_col; i++)
    CHECK (((unsigned char *)small_col)[i] == '.');
  for (size_t i = 0; i < 6 * sizeof *small_val; i++)
    CHECK (((unsigned char *)small_val)[i] == '.');
  /* what acm_tally_batch runs on the host: the loop into a record room of its own, then the pass above */
  uint64_t total = 99;
  nnz = 99;
  memset (row_ptr, 0xFF, (n_texts + 1) * sizeof *row_ptr);
  memset (col, 0xFF, 7 * sizeof *col);
  memset (val, 0xFF, 7 * sizeof *val);
  CHECK (acm_internal_cpu_tally_batch (m, text, off, n_texts, 3, row_ptr, col, val, 7, &nnz, &total) == ACM_GPU_OK);
  CHECK (nnz == 7 && total == 10 && memcmp (row_ptr, want_ptr, sizeof want_ptr) == 0);
  CHECK (memcmp (col, want_col, sizeof want_col) == 0 && memcmp (val, want_val, sizeof want_val) == 0);
  /* "he", 3000 x "s", "she": more records than the 1024 the room starts with, so it is grown */
  unsigned char *big = malloc (3 * 3005);
  CHECK (big);
  sym3 (big, "he", 2);
  for (int i = 0; i < 3000; i++)
    sym3 (big + 3 * (2 + i), "s", 1);
  sym3 (big + 3 * 3002, "she", 3);
  uint64_t *big_off = exact ((uint64_t[]){ 0, 2, 3002, 3005 }, 4 * sizeof (uint64_t));
  uint64_t *big_ptr = malloc (4 * sizeof *big_ptr), *big_val = malloc (5 * sizeof *big_val);
  uint32_t *big_col = malloc (5 * sizeof *big_col);
  CHECK (big_ptr && big_val && big_col);
  CHECK (acm_internal_cpu_tally_batch (m, big, big_off, 3, 3, big_ptr, big_col, big_val, 5, &nnz, &total) == ACM_GPU_OK);
  CHECK (nnz == 5 && total == 3004 && memcmp (big_ptr, (uint64_t[]){ 0, 1, 2, 5 }, 4 * sizeof (uint64_t)) == 0);
  CHECK (memcmp (big_col, (uint32_t[]){ 0, 3, 0, 1, 3 }, 5 * sizeof (uint32_t)) == 0);
  CHECK (memcmp (big_val, (uint64_t[]){ 1, 3000, 1, 1, 1 }, 5 * sizeof (uint64_t)) == 0);
  free (big_col), free (big_val), free (big_ptr), free (big_off), free (big);
  /* counting only; no text at all; a first[] that decreases; a keyword id that is none */
  nnz = 99;
  CHECK (acm_tally_batch_records (records, first, n_texts, 4, row_ptr, NULL, NULL, 0, &nnz) == ACM_GPU_OK && nnz == 7);
  uint64_t *zero = exact ((uint64_t[]){ 0 }, sizeof (uint64_t));
  uint64_t *one_ptr = malloc (sizeof *one_ptr);
  CHECK (one_ptr);
  *one_ptr = 77;
  CHECK (acm_tally_batch_records (NULL, zero, 0, 4, one_ptr, NULL, NULL, 0, &nnz) == ACM_GPU_OK && nnz == 0 && *one_ptr == 0);
  CHECK (acm_tally_batch_records (records, first, n_texts, 3, row_ptr, col, val, 7, &nnz) == ACM_GPU_E_ARG);
  first[2] = 6; /* (first[3] = 5) */
  CHECK (acm_tally_batch_records (records, first, n_texts, 4, row_ptr, col, val, 7, &nnz) == ACM_GPU_E_ARG);
  free (one_ptr), free (zero), free (small_val), free (small_col), free (val), free (col), free (row_ptr), free (first), free (records), free (off),
    free (text);
  acm_release (m);
  for (int k = 0; k < 4; k++)
    free (letters[k]);
  printf ("all checks held\n");
  return 0;
}
