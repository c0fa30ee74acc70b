/* Test-only driver: acm_context_records and acm_context's host path, acm_internal_cpu_context (acm_host.c,
 * no HIP), under AddressSanitizer and UBSan -- nested and touching windows, a batch with empty texts and a
 * record across a cut, windows that saturate, an output with one symbol too little room, 8-byte symbols.
 * Every buffer is allocated at its exact size, so that a byte read or written beside it is seen.  Built
 * and run by tests/test_context_sanitized.py; exits 0 when every check held. */
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
  /* "she hehe x he" with {he, she, his, hers}: she+he nested, hehe touching, he alone -- (end_pos, length, keyword) */
  const ACMRecord found[5] = { { 2, 3, 1 }, { 2, 2, 0 }, { 5, 2, 0 }, { 7, 2, 0 }, { 12, 2, 0 } };
  char *text = exact ("she hehe x he", 13);
  ACMRecord *rec = exact (found, sizeof found);
  uint64_t *snip_lo = malloc (5 * 8), *out_off = malloc (6 * 8);
  uint32_t *snip_text = malloc (5 * 4), *rec_snip = malloc (5 * 4);
  int64_t *rec_at = malloc (5 * 8);
  char *out = malloc (9);
  CHECK (snip_lo && out_off && snip_text && rec_snip && rec_at && out);
  uint64_t ns = 99, sym = 99;
  CHECK (acm_context_records (text, 13, 1, 0, NULL, 0, rec, 5, 0, 0, ACM_CONTEXT_MERGE, out, 9, &sym, &ns, snip_lo, out_off, snip_text, rec_snip,
                              rec_at) == ACM_GPU_OK);
  CHECK (ns == 3 && sym == 9 && memcmp (out, "shehehehe", 9) == 0);
  CHECK (snip_lo[0] == 0 && snip_lo[1] == 4 && snip_lo[2] == 11 && out_off[0] == 0 && out_off[1] == 3 && out_off[2] == 7 && out_off[3] == 9);
  CHECK (rec_snip[0] == 0 && rec_snip[1] == 0 && rec_snip[2] == 1 && rec_snip[3] == 1 && rec_snip[4] == 2);
  CHECK (rec_at[0] == 0 && rec_at[1] == 1 && rec_at[2] == 3 && rec_at[3] == 5 && rec_at[4] == 7 && snip_text[2] == 0);
  /* one symbol too little room: the need, nothing written, the arrays valid */
  char *small = malloc (8);
  CHECK (small);
  memset (small, '.', 8);
  memset (out_off, 0xFF, 6 * 8);
  CHECK (acm_context_records (text, 13, 1, 0, NULL, 0, rec, 5, 0, 0, ACM_CONTEXT_MERGE, small, 8, &sym, &ns, snip_lo, out_off, NULL, NULL, NULL) ==
         ACM_GPU_E_OVERFLOW);
  CHECK (ns == 3 && sym == 9 && memcmp (small, "........", 8) == 0 && out_off[3] == 9);
  /* windows that saturate: the whole text, once (MERGE) and per record (EACH, no output buffer: the length alone) */
  char *whole = malloc (13);
  CHECK (whole);
  CHECK (acm_context_records (text, 13, 1, 0, NULL, 0, rec, 5, 0xFFFFFFFFu, 0xFFFFFFFFu, ACM_CONTEXT_MERGE, whole, 13, &sym, &ns, snip_lo, out_off, NULL,
                              rec_snip, rec_at) == ACM_GPU_OK);
  CHECK (ns == 1 && sym == 13 && memcmp (whole, text, 13) == 0 && rec_at[4] == 11);
  CHECK (acm_context_records (text, 13, 1, 0, NULL, 0, rec, 5, 0xFFFFFFFFu, 0xFFFFFFFFu, ACM_CONTEXT_EACH, NULL, 0, &sym, &ns, NULL, NULL, NULL, NULL,
                              NULL) == ACM_GPU_OK);
  CHECK (ns == 5 && sym == 65);
  /* a batch: "" | "ushers" | "" | "he" | "us" | "hers" | "" -- `she` of us|hers spans a cut; TEXTS reaches past both ends */
  char *packed = exact ("ushersheushers", 14);
  uint64_t *off = exact ((uint64_t[]){ 0, 0, 6, 6, 8, 10, 14, 14 }, 8 * sizeof (uint64_t));
  const ACMRecord batch[7] = { { 3, 3, 1 }, { 3, 2, 0 }, { 5, 4, 3 }, { 7, 2, 0 }, { 11, 3, 1 }, { 11, 2, 0 }, { 13, 4, 3 } };
  ACMRecord *brec = exact (batch, sizeof batch);
  uint64_t *blo = malloc (7 * 8), *boff = malloc (8 * 8);
  uint32_t *btext = malloc (7 * 4), *bsnip = malloc (7 * 4);
  int64_t *bat = malloc (7 * 8);
  char *bout = malloc (14);
  CHECK (blo && boff && btext && bsnip && bat && bout);
  CHECK (acm_context_records (packed, 14, 1, 0, off, 7, brec, 7, 1, 0, ACM_CONTEXT_MERGE, bout, 14, &sym, &ns, blo, boff, btext, bsnip, bat) == ACM_GPU_OK);
  /* ushers -> [0, 6); he -> [6, 8) touches it across a boundary: two snippets; hers -> [10, 14) */
  CHECK (ns == 3 && sym == 12 && memcmp (bout, "ushershehers", 12) == 0 && blo[1] == 6 && btext[0] == 1 && btext[1] == 3 && btext[2] == 5);
  CHECK (bsnip[4] == ACM_CONTEXT_NONE && bat[4] == -1 && bsnip[5] == 2 && bat[5] == 8);
  CHECK (acm_context_records (packed, 14, 1, 0, off, 7, brec, 7, 0, 0, ACM_CONTEXT_TEXTS | ACM_CONTEXT_MERGE, bout, 14, &sym, &ns, blo, boff, btext,
                              bsnip, bat) == ACM_GPU_OK);
  CHECK (ns == 2 && sym == 12 && blo[0] == 0 && blo[1] == 10 && btext[0] == 1 && btext[1] == 5);
  CHECK (acm_context_records (packed, 14, 1, 0, off, 7, brec, 7, 0xFFFFFFFFu, 0xFFFFFFFFu, ACM_CONTEXT_TEXTS | ACM_CONTEXT_EACH, NULL, 0, &sym, &ns, blo,
                              boff, btext, bsnip, bat) == ACM_GPU_OK);
  CHECK (ns == 7 && sym == 6 * 14 && blo[4] == 9 && boff[5] - boff[4] == 0 && btext[4] == 4 && btext[0] == 1);
  /* the contract */
  CHECK (acm_context_records (packed, 14, 1, 0, off, 7, brec, 7, 0, 0, 4, NULL, 0, &sym, &ns, NULL, NULL, NULL, NULL, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_context_records (packed, 14, 1, 0, NULL, 0, brec, 7, 0, 0, ACM_CONTEXT_TEXTS, NULL, 0, &sym, &ns, NULL, NULL, NULL, NULL, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_context_records (packed, 13, 1, 0, off, 7, brec, 7, 0, 0, 0, NULL, 0, &sym, &ns, NULL, NULL, NULL, NULL, NULL) == ACM_GPU_E_ARG);
  brec[2] = (ACMRecord){ 2, 2, 0 }; /* end_pos decreases: MERGE refuses, EACH does not */
  CHECK (acm_context_records (packed, 14, 1, 0, off, 7, brec, 7, 0, 0, ACM_CONTEXT_MERGE, NULL, 0, &sym, &ns, NULL, NULL, NULL, NULL, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_context_records (packed, 14, 1, 0, off, 7, brec, 7, 0, 0, ACM_CONTEXT_EACH, NULL, 0, &sym, &ns, NULL, NULL, NULL, NULL, NULL) == ACM_GPU_OK);
  brec[2].end_pos = 14; /* beyond the buffer */
  CHECK (acm_context_records (packed, 14, 1, 0, off, 7, brec, 7, 0, 0, ACM_CONTEXT_EACH, NULL, 0, &sym, &ns, NULL, NULL, NULL, NULL, NULL) == ACM_GPU_E_ARG);
  /* symbols of 8 bytes with pos_base, no records at all */
  uint64_t *t8 = malloc (13 * 8), *o8 = malloc (9 * 8);
  CHECK (t8 && o8);
  for (int i = 0; i < 13; i++)
    t8[i] = 0x4100000000000000ull | (unsigned char)text[i];
  for (int i = 0; i < 5; i++)
    rec[i].end_pos += 1ull << 40;
  CHECK (acm_context_records (t8, 13, 8, 1ull << 40, NULL, 0, rec, 5, 0, 0, ACM_CONTEXT_MERGE, o8, 9, &sym, &ns, snip_lo, out_off, NULL, NULL, rec_at) ==
         ACM_GPU_OK);
  CHECK (ns == 3 && sym == 9 && o8[3] == t8[4] && o8[8] == t8[12] && rec_at[4] == 7);
  CHECK (acm_context_records (t8, 13, 8, 0, NULL, 0, NULL, 0, 3, 3, ACM_CONTEXT_MERGE, o8, 9, &sym, &ns, snip_lo, out_off, NULL, NULL, NULL) == ACM_GPU_OK);
  CHECK (ns == 0 && sym == 0 && out_off[0] == 0);
  /* what acm_context runs on the host for a machine no GPU path takes: the caller loop, then the pass above -- into the
   * caller's record room and into one of its own; a room one record short */
  ACMachine *m = acm_create (ACM_CMP_DEFAULT, &(size_t){ 1 }, 0);
  const char *words[4] = { "he", "she", "his", "hers" };
  for (int k = 0; k < 4; k++) {
    const ACState *s = acm_initiate (m);
    for (const char *c = words[k]; *c; c++)
      acm_insert_letter_of_keyword (&s, (void *)c);
    acm_insert_end_of_keyword (&s, 0, 0);
  }
  uint64_t n = 99;
  ACMRecord *room = malloc (5 * sizeof *room);
  CHECK (room);
  for (int own = 0; own < 2; own++) {
    CHECK (acm_internal_cpu_context (m, text, 13, 1, own ? NULL : room, 5, &n, 1, 1, ACM_CONTEXT_MERGE, out, 9, &sym, &ns, snip_lo, out_off, snip_text,
                                     rec_snip, rec_at) == ACM_GPU_E_OVERFLOW);
    CHECK (n == 5 && ns == 2 && sym == 12 && out_off[1] == 9 && snip_lo[1] == 10); /* "she hehe " and " he": the output's room is short */
  }
  char *out12 = malloc (12);
  CHECK (out12);
  CHECK (acm_internal_cpu_context (m, text, 13, 1, room, 5, &n, 1, 1, ACM_CONTEXT_MERGE, out12, 12, &sym, &ns, snip_lo, out_off, snip_text, rec_snip,
                                   rec_at) == ACM_GPU_OK);
  CHECK (n == 5 && memcmp (out12, "she hehe  he", 12) == 0 && room[4].end_pos == 12 && rec_at[4] == 10);
  CHECK (acm_internal_cpu_context (m, text, 13, 1, room, 4, &n, 1, 1, ACM_CONTEXT_MERGE, out12, 12, &sym, &ns, snip_lo, out_off, snip_text, rec_snip,
                                   rec_at) == ACM_GPU_E_OVERFLOW);
  CHECK (n == 5);
  acm_release (m);
  free (out12), free (room), free (o8), free (t8), free (bout), free (bat), free (bsnip), free (btext), free (boff), free (blo), free (brec), free (off);
  free (packed), free (whole), free (small), free (out), free (rec_at), free (rec_snip), free (snip_text), free (out_off), free (snip_lo), free (rec);
  free (text);
  printf ("all checks held\n");
  return 0;
}
