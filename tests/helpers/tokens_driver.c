/* Test-only driver: acm_tokens_records and acm_tokenize's host path, acm_internal_cpu_tokenize
 * (acm_host.c, no HIP), under AddressSanitizer and UBSan -- the ushers case in the three modes, as one
 * text and as the batch us | hers, a count-only call, a token room one short, the argument errors, a
 * text with more records than the host path's record room starts with.  Every buffer is allocated at its
 * exact size, so that a byte read or written beside it is seen.  Built and run by
 * tests/test_tokens_sanitized.py; exits 0 when every check held. */
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

static int
same32 (const uint32_t *a, const uint32_t *b, size_t n) {
  return memcmp (a, b, n * sizeof *a) == 0;
}

static int
same64 (const uint64_t *a, const uint64_t *b, size_t n) {
  return memcmp (a, b, n * sizeof *a) == 0;
}

int
main (void) {
  /* `ushers` with {he, she, his, hers}: the caller loop through the machine, then the selection */
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
  const uint32_t gb = 1000;
  uint64_t need = 99;
  /* SYMBOL: four tokens, every array at its exact size */
  uint32_t *id = malloc (4 * sizeof *id), *len = malloc (4 * sizeof *len);
  uint64_t *start = malloc (4 * sizeof *start);
  CHECK (id && len && start);
  CHECK (acm_tokens_records (text, 6, 1, 0, rec, n, NULL, 0, NULL, 0, gb, ACM_TOKENS_GAP_SYMBOL, id, start, len, 4, &need, NULL) == ACM_GPU_OK);
  CHECK (need == 4 && same32 (id, (uint32_t[]){ gb + 'u', 1, gb + 'r', gb + 's' }, 4) && same64 (start, (uint64_t[]){ 0, 1, 4, 5 }, 4) &&
         same32 (len, (uint32_t[]){ 1, 3, 1, 1 }, 4));
  /* one token too little room: the need, nothing written */
  memset (id, 0x2e, 3 * sizeof *id);
  need = 99;
  CHECK (acm_tokens_records (text, 6, 1, 0, rec, n, NULL, 0, NULL, 0, gb, ACM_TOKENS_GAP_SYMBOL, id, start, len, 3, &need, NULL) == ACM_GPU_E_OVERFLOW);
  CHECK (need == 4 && id[0] == 0x2e2e2e2e && id[2] == 0x2e2e2e2e);
  /* RUN through a table keyword -> vocabulary id of exactly four entries; start and length are optional */
  uint32_t *tok_of = exact ((uint32_t[]){ 50, 51, 52, 53 }, 4 * sizeof (uint32_t));
  CHECK (acm_tokens_records (NULL, 6, 1, 0, rec, n, NULL, 0, tok_of, 4, gb, ACM_TOKENS_GAP_RUN, id, NULL, len, 3, &need, NULL) == ACM_GPU_OK);
  CHECK (need == 3 && same32 (id, (uint32_t[]){ gb, 51, gb }, 3) && same32 (len, (uint32_t[]){ 1, 3, 2 }, 3));
  CHECK (acm_tokens_records (NULL, 6, 1, 0, rec, n, NULL, 0, tok_of, 4, gb, ACM_TOKENS_GAP_DROP, id, start, NULL, 1, &need, NULL) == ACM_GPU_OK);
  CHECK (need == 1 && id[0] == 51 && start[0] == 1);
  /* a count-only call ignores the capacity and needs no array */
  need = 99;
  CHECK (acm_tokens_records (NULL, 6, 1, 0, rec, n, NULL, 0, NULL, 0, gb, ACM_TOKENS_GAP_RUN, NULL, NULL, NULL, 0, &need, NULL) == ACM_GPU_OK && need == 3);
  /* the batch us | hers: the records of `hers` alone are he (end 3) and hers (end 5); SELECT keeps hers */
  ACMRecord *brec = exact ((ACMRecord[]){ { 3, 2, 0 }, { 5, 4, 3 } }, 2 * sizeof (ACMRecord));
  uint64_t bn = acm_select_records (brec, 2);
  CHECK (bn == 1 && brec[0].end_pos == 5 && brec[0].keyword_id == 3);
  uint64_t *off = exact ((uint64_t[]){ 0, 2, 6 }, 3 * sizeof (uint64_t));
  uint64_t *first = malloc (3 * sizeof *first);
  CHECK (first);
  CHECK (acm_tokens_records (NULL, 6, 1, 0, brec, bn, off, 2, NULL, 0, gb, ACM_TOKENS_GAP_RUN, id, start, len, 2, &need, first) == ACM_GPU_OK);
  CHECK (need == 2 && same32 (id, (uint32_t[]){ gb, 3 }, 2) && same64 (start, (uint64_t[]){ 0, 2 }, 2) && same32 (len, (uint32_t[]){ 2, 4 }, 2) &&
         same64 (first, (uint64_t[]){ 0, 1, 2 }, 3));
  /* what acm_tokenize runs on the host for a machine no GPU path takes (the loop into a record room of its
   * own, the selection, the pass above): the one text through the table, then the batch */
  uint64_t selected = 99;
  CHECK (acm_internal_cpu_tokenize (m, text, 6, 1, NULL, 0, tok_of, 4, gb, ACM_TOKENS_GAP_RUN, id, NULL, len, 3, &need, NULL, &selected) == ACM_GPU_OK);
  CHECK (need == 3 && selected == 1 && same32 (id, (uint32_t[]){ gb, 51, gb }, 3) && same32 (len, (uint32_t[]){ 1, 3, 2 }, 3));
  memset (first, 0xff, 3 * sizeof *first);
  CHECK (acm_internal_cpu_tokenize (m, text, 6, 1, off, 2, NULL, 0, gb, ACM_TOKENS_GAP_RUN, id, start, len, 2, &need, first, &selected) == ACM_GPU_OK);
  CHECK (need == 2 && selected == 1 && same32 (id, (uint32_t[]){ gb, 3 }, 2) && same64 (start, (uint64_t[]){ 0, 2 }, 2) &&
         same32 (len, (uint32_t[]){ 2, 4 }, 2) && same64 (first, (uint64_t[]){ 0, 1, 2 }, 3));
  /* "he" x 1500: more records than the 1024 the room starts with, so it is grown; 1500 tokens of `he` and no gap */
  char *big = malloc (3000);
  uint32_t *big_id = malloc (1500 * sizeof *big_id);
  uint64_t *big_start = malloc (1500 * sizeof *big_start);
  CHECK (big && big_id && big_start);
  for (int i = 0; i < 3000; i++)
    big[i] = "he"[i % 2];
  CHECK (acm_internal_cpu_tokenize (m, big, 3000, 1, NULL, 0, tok_of, 4, gb, ACM_TOKENS_GAP_DROP, big_id, big_start, NULL, 1500, &need, NULL, &selected) ==
         ACM_GPU_OK);
  CHECK (need == 1500 && selected == 1500);
  for (uint64_t i = 0; i < 1500; i++)
    CHECK (big_id[i] == 50 && big_start[i] == 2 * i);
  free (big_start), free (big_id), free (big);
  /* the token room too small: tok_first is written all the same */
  memset (first, 0xff, 3 * sizeof *first);
  CHECK (acm_tokens_records (text, 6, 1, 0, brec, bn, off, 2, NULL, 0, gb, ACM_TOKENS_GAP_SYMBOL, id, start, len, 2, &need, first) == ACM_GPU_E_OVERFLOW);
  CHECK (need == 3 && same64 (first, (uint64_t[]){ 0, 2, 3 }, 3));
  /* abcd without a match as ab | cd, with two empty texts at the end: no record array at all */
  uint64_t *off4 = exact ((uint64_t[]){ 0, 2, 4, 4, 4 }, 5 * sizeof (uint64_t));
  uint64_t *first4 = malloc (5 * sizeof *first4);
  CHECK (first4);
  CHECK (acm_tokens_records (NULL, 4, 1, 0, NULL, 0, off4, 4, NULL, 0, gb, ACM_TOKENS_GAP_RUN, id, start, len, 2, &need, first4) == ACM_GPU_OK);
  CHECK (need == 2 && same64 (start, (uint64_t[]){ 0, 2 }, 2) && same64 (first4, (uint64_t[]){ 0, 1, 2, 2, 2 }, 5));
  /* symbols of 2 bytes in SYMBOL mode, pos_base in the records' coordinate */
  unsigned char *t2 = exact ((unsigned char[]){ 0x02, 0x01, 0xff, 0xff, 0x61, 0x00 }, 6);
  ACMRecord *r2 = exact ((ACMRecord[]){ { 1002, 1, 0 } }, sizeof (ACMRecord));
  CHECK (acm_tokens_records (t2, 3, 2, 1000, r2, 1, NULL, 0, NULL, 0, 0xffff0000u, ACM_TOKENS_GAP_SYMBOL, id, start, len, 3, &need, NULL) == ACM_GPU_OK);
  CHECK (need == 3 && same32 (id, (uint32_t[]){ 0xffff0102u, 0xffffffffu, 0 }, 3) && same64 (start, (uint64_t[]){ 1000, 1001, 1002 }, 3));
  /* the argument errors: nothing is read behind an array */
  CHECK (acm_tokens_records (t2, 3, 2, 1000, r2, 1, NULL, 0, NULL, 0, 0xffff0001u, ACM_TOKENS_GAP_SYMBOL, id, start, len, 3, &need, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_tokens_records (t2, 3, 2, 0, r2, 1, NULL, 0, NULL, 0, 0, ACM_TOKENS_GAP_RUN, id, start, len, 3, &need, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_tokens_records (text, 6, 1, 0, rec, n, NULL, 0, tok_of, 1, gb, ACM_TOKENS_GAP_RUN, id, start, len, 4, &need, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_tokens_records (text, 6, 1, 0, rec, n, off, 2, NULL, 0, gb, ACM_TOKENS_GAP_RUN, id, start, len, 4, &need, first) == ACM_GPU_E_ARG);
  CHECK (acm_tokens_records (text, 6, 1, 0, rec, n, NULL, 0, NULL, 0, gb, 3, id, start, len, 4, &need, NULL) == ACM_GPU_E_ARG);
  off[1] = 7;
  CHECK (acm_tokens_records (text, 6, 1, 0, brec, bn, off, 2, NULL, 0, gb, ACM_TOKENS_GAP_RUN, id, start, len, 4, &need, first) == ACM_GPU_E_ARG);
  free (r2), free (t2), free (first4), free (off4), free (first), free (off), free (brec), free (tok_of), free (start), free (len), free (id), free (rec),
    free (text);
  acm_release (m);
  printf ("all checks held\n");
  return 0;
}
