/* Test-only driver: acm_replace_records and acm_replace's host path, acm_internal_cpu_replace (acm_host.c,
 * no HIP), under AddressSanitizer and UBSan -- the ushers case, a deletion of everything, an output with
 * one symbol too little room, a text with more records than the host path's record room starts with.
 * Every buffer is allocated at its exact size, so that a byte read or written beside it is seen.  Built
 * and run by tests/test_replace_sanitized.py; exits 0 when every check held. */
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

int
main (void) {
  /* `ushers` with {he, she, his, hers}: the caller loop through the machine, the selection, the replacement */
  ACMachine *m = acm_create (ACM_CMP_DEFAULT, &(size_t){ 1 }, 0);
  const char *words[4] = { "he", "she", "his", "hers" };
  for (int k = 0; k < 4; k++) {
    const ACState *s = acm_initiate (m);
    for (const char *c = words[k]; *c; c++)
      acm_insert_letter_of_keyword (&s, (void *)c);
    acm_insert_end_of_keyword (&s, 0, 0);
  }
  char *text = exact ("ushers", 6);
  ACMRecord *rec = malloc (3 * sizeof *rec);
  CHECK (rec);
  uint64_t n = 0;
  const ACState *s = acm_initiate (m);
  for (uint64_t i = 0; i < 6; i++) {
    const size_t nb = acm_match (&s, &text[i]);
    MatchHolder h;
    acm_matcher_init (&h);
    for (size_t j = 0; j < nb; j++) {
      acm_get_match (s, j, &h);
      CHECK (n < 3);
      rec[n].end_pos = i;
      rec[n].length = (uint32_t)h.length;
      rec[n].keyword_id = h.length == 3 ? 1 : h.length == 2 ? 0 : 3;
      n++;
    }
    acm_matcher_release (&h);
  }
  CHECK (n == 3);
  n = acm_select_records (rec, n);
  CHECK (n == 1 && rec[0].end_pos == 3 && rec[0].length == 3 && rec[0].keyword_id == 1);
  char *data = exact ("[H][X][I][R]", 12);
  uint64_t *off = exact ((uint64_t[]){ 0, 3, 6, 9, 12 }, 5 * sizeof (uint64_t));
  char *out = malloc (6);
  CHECK (out);
  uint64_t need = 99;
  CHECK (acm_replace_records (text, 6, 1, 0, rec, n, data, off, 4, out, 6, &need) == ACM_GPU_OK);
  CHECK (need == 6 && memcmp (out, "u[X]rs", 6) == 0);
  /* one symbol too little room: the need, nothing written */
  char *small = malloc (5);
  CHECK (small);
  memset (small, '.', 5);
  need = 99;
  CHECK (acm_replace_records (text, 6, 1, 0, rec, n, data, off, 4, small, 5, &need) == ACM_GPU_E_OVERFLOW);
  CHECK (need == 6 && memcmp (small, ".....", 5) == 0);
  /* masked, in place of the table */
  CHECK (acm_replace_records (text, 6, 1, 0, rec, n, "*", NULL, 0, out, 6, &need) == ACM_GPU_OK);
  CHECK (need == 6 && memcmp (out, "u***rs", 6) == 0);
  /* a keyword id the table does not have, a record beyond the text */
  CHECK (acm_replace_records (text, 6, 1, 0, rec, n, data, off, 1, out, 6, &need) == ACM_GPU_E_ARG);
  CHECK (acm_replace_records (text, 3, 1, 0, rec, n, data, off, 4, out, 6, &need) == ACM_GPU_E_ARG);
  /* deletion of everything: {a} on aaaa with an empty replacement, symbols of 3 bytes, no output buffer at all */
  unsigned char *t3 = malloc (12);
  CHECK (t3);
  for (int i = 0; i < 12; i++)
    t3[i] = (unsigned char)("a\x3b\x07"[i % 3]);
  ACMRecord *all = malloc (4 * sizeof *all);
  CHECK (all);
  for (int i = 0; i < 4; i++)
    all[i] = (ACMRecord){ 1000 + (uint64_t)i, 1, 0 };
  uint64_t *off0 = exact ((uint64_t[]){ 0, 0 }, 2 * sizeof (uint64_t));
  need = 99;
  CHECK (acm_replace_records (t3, 4, 3, 1000, all, 4, NULL, off0, 1, NULL, 0, &need) == ACM_GPU_OK && need == 0);
  /* the same selection with a replacement of two symbols: the output is twice the text */
  unsigned char *r3 = malloc (6), *o3 = malloc (24);
  CHECK (r3 && o3);
  memcpy (r3, "XYZxyz", 6);
  off0[1] = 2;
  CHECK (acm_replace_records (t3, 4, 3, 1000, all, 4, r3, off0, 1, o3, 8, &need) == ACM_GPU_OK && need == 8);
  for (int i = 0; i < 4; i++)
    CHECK (memcmp (o3 + 6 * i, "XYZxyz", 6) == 0);
  /* what acm_replace runs on the host for a machine no GPU path takes: the loop into a record room of
   * its own, the selection, the pass above */
  uint64_t replaced = 99;
  need = 99;
  CHECK (acm_internal_cpu_replace (m, text, 6, 1, data, off, 4, out, 6, &need, &replaced) == ACM_GPU_OK);
  CHECK (need == 6 && replaced == 1 && memcmp (out, "u[X]rs", 6) == 0);
  /* "he" x 1500: more records than the 1024 the room starts with, so it is grown; every match becomes "[H]" */
  char *big = malloc (3000), *big_out = malloc (4500);
  CHECK (big && big_out);
  for (int i = 0; i < 3000; i++)
    big[i] = "he"[i % 2];
  CHECK (acm_internal_cpu_replace (m, big, 3000, 1, data, off, 4, big_out, 4500, &need, &replaced) == ACM_GPU_OK);
  CHECK (need == 4500 && replaced == 1500);
  for (int i = 0; i < 4500; i++)
    CHECK (big_out[i] == "[H]"[i % 3]);
  free (big_out), free (big);
  free (o3), free (r3), free (off0), free (all), free (t3), free (small), free (out), free (off), free (data), free (rec), free (text);
  acm_release (m);
  printf ("all checks held\n");
  return 0;
}
