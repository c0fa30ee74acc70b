/* Test-only driver: acm_rules_check, acm_rules_matrix and acm_rules' host path (acm_host.c, no HIP)
 * under AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte
 * read or written beside it is seen.  The machine's comparator is memcmp over 3-byte symbols,
 * declared with acm_set_symbol_bytes: what acm_rules runs for it is the caller loop on the host,
 * acm_internal_cpu_rules (acm_rules itself lives in the HIP translation unit, which this program
 * does not link).  Built and run by tests/test_rules_sanitized.py; exits 0 when every check held. */
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

#define NO_MAX ACM_RULE_NO_MAX

int
main (void) {
  /* the count matrix of {he, she, hers, s} (ids 0, 1, 2, 3) over the texts "", "us", "hers and sh", "e sells she", "",
   * "on top", "": us: s | hers and sh: he, hers, s x 2 | e sells she: he, she, s x 3 */
  const uint64_t n_texts = 7;
  uint64_t *row_ptr = exact ((uint64_t[]){ 0, 0, 1, 4, 7, 7, 7, 7 }, 8 * sizeof (uint64_t));
  uint32_t *col = exact ((uint32_t[]){ 3, 0, 2, 3, 0, 1, 3 }, 7 * sizeof (uint32_t));
  uint64_t *val = exact ((uint64_t[]){ 1, 1, 1, 2, 1, 1, 3 }, 7 * sizeof (uint64_t));
  /* 0: he and hers | 1: she or hers | 2: s and not he | 3: not he (an always-rule) | 4: s in [2, 2] or s >= 3, one keyword
   * twice | 5: 2 of {he, she, hers, s >= 2} | 6: she at any count and s >= 3 */
  const ACMRuleTerm all_terms[14] = { { 0, 1, NO_MAX }, { 2, 1, NO_MAX }, { 1, 1, NO_MAX }, { 2, 1, NO_MAX }, { 3, 1, NO_MAX }, { 0, 0, 0 },
                                      { 0, 0, 0 },      { 3, 2, 2 },      { 3, 3, NO_MAX }, { 0, 1, NO_MAX }, { 1, 1, NO_MAX }, { 2, 1, NO_MAX },
                                      { 3, 2, NO_MAX }, { 1, 0, NO_MAX } };
  /* (the last rule has two terms: the fifteenth is added below) */
  ACMRuleTerm *terms = malloc (15 * sizeof *terms);
  CHECK (terms);
  memcpy (terms, all_terms, sizeof all_terms);
  terms[14] = (ACMRuleTerm){ 3, 3, NO_MAX };
  uint64_t *rule_ptr = exact ((uint64_t[]){ 0, 2, 4, 6, 7, 9, 13, 15 }, 8 * sizeof (uint64_t));
  uint32_t *need = exact ((uint32_t[]){ 2, 1, 2, 1, 1, 2, 2 }, 7 * sizeof (uint32_t));
  const uint64_t n_rules = 7;
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 4) == ACM_GPU_OK);
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 3) == ACM_GPU_E_ARG); /* keyword 3 is none then */
  /* "": 3 | us: 2, 3 | hers and sh: 0, 1, 4, 5 | e sells she: 1, 4, 5, 6 | "": 3 | on top: 3 | "": 3 */
  const uint64_t want_ptr[8] = { 0, 1, 3, 7, 11, 12, 13, 14 };
  const uint32_t want[14] = { 3, 2, 3, 0, 1, 4, 5, 1, 4, 5, 6, 3, 3, 3 };
  uint64_t *fired_ptr = malloc ((n_texts + 1) * sizeof *fired_ptr);
  uint32_t *fired = malloc (14 * sizeof *fired);
  CHECK (fired_ptr && fired);
  uint64_t n_fired = 99;
  CHECK (acm_rules_matrix (row_ptr, col, val, n_texts, 4, terms, rule_ptr, need, n_rules, fired_ptr, fired, 14, &n_fired) == ACM_GPU_OK);
  CHECK (n_fired == 14 && memcmp (fired_ptr, want_ptr, sizeof want_ptr) == 0 && memcmp (fired, want, sizeof want) == 0);
  /* one entry too little room: the need, nothing written to fired, fired_ptr all the same */
  uint32_t *small = malloc (13 * sizeof *small);
  CHECK (small);
  memset (small, '.', 13 * sizeof *small);
  memset (fired_ptr, 0xFF, (n_texts + 1) * sizeof *fired_ptr);
  n_fired = 99;
  CHECK (acm_rules_matrix (row_ptr, col, val, n_texts, 4, terms, rule_ptr, need, n_rules, fired_ptr, small, 13, &n_fired) == ACM_GPU_E_OVERFLOW);
  CHECK (n_fired == 14 && memcmp (fired_ptr, want_ptr, sizeof want_ptr) == 0);
  for (size_t i = 0; i < 13 * sizeof *small; i++)
    CHECK (((unsigned char *)small)[i] == '.');
  /* counting only; no text at all; no rule at all */
  n_fired = 99;
  CHECK (acm_rules_matrix (row_ptr, col, val, n_texts, 4, terms, rule_ptr, need, n_rules, fired_ptr, NULL, 0, &n_fired) == ACM_GPU_OK && n_fired == 14);
  uint64_t *zero = exact ((uint64_t[]){ 0 }, sizeof (uint64_t));
  uint64_t *one_ptr = malloc (sizeof *one_ptr);
  CHECK (one_ptr);
  *one_ptr = 77;
  CHECK (acm_rules_matrix (zero, NULL, NULL, 0, 4, terms, rule_ptr, need, n_rules, one_ptr, NULL, 0, &n_fired) == ACM_GPU_OK && n_fired == 0 && *one_ptr == 0);
  CHECK (acm_rules_matrix (row_ptr, col, val, n_texts, 4, NULL, zero, NULL, 0, fired_ptr, fired, 14, &n_fired) == ACM_GPU_OK && n_fired == 0);
  for (uint64_t t = 0; t <= n_texts; t++)
    CHECK (fired_ptr[t] == 0);
  /* a count above 2^32 holds a term without an upper bound and fails one with the largest bound there is */
  uint64_t *big_ptr = exact ((uint64_t[]){ 0, 1 }, 2 * sizeof (uint64_t));
  uint32_t *big_col = exact ((uint32_t[]){ 1 }, sizeof (uint32_t));
  uint64_t *big_val = exact ((uint64_t[]){ (1ull << 32) + 5 }, sizeof (uint64_t));
  ACMRuleTerm *big_terms = exact ((ACMRuleTerm[]){ { 1, 1, NO_MAX }, { 1, 1, 0xFFFFFFFEu } }, 2 * sizeof (ACMRuleTerm));
  uint64_t *big_rule_ptr = exact ((uint64_t[]){ 0, 1, 2 }, 3 * sizeof (uint64_t));
  uint32_t *big_need = exact ((uint32_t[]){ 1, 1 }, 2 * sizeof (uint32_t));
  uint64_t *big_fired_ptr = malloc (2 * sizeof *big_fired_ptr);
  uint32_t *big_fired = malloc (sizeof *big_fired);
  CHECK (big_fired_ptr && big_fired);
  CHECK (acm_rules_matrix (big_ptr, big_col, big_val, 1, 2, big_terms, big_rule_ptr, big_need, 2, big_fired_ptr, big_fired, 1, &n_fired) == ACM_GPU_OK);
  CHECK (n_fired == 1 && big_fired[0] == 0 && big_fired_ptr[1] == 1);
  /* the refusals: a row_ptr that decreases, one that does not begin with 0, a col that is no keyword; a rule without
   * terms, need 0, need above the terms, lo > hi, a rule_ptr that does not begin with 0 */
  row_ptr[2] = 5; /* (row_ptr[3] = 4) */
  CHECK (acm_rules_matrix (row_ptr, col, val, n_texts, 4, terms, rule_ptr, need, n_rules, fired_ptr, fired, 14, &n_fired) == ACM_GPU_E_ARG);
  row_ptr[2] = 1;
  row_ptr[0] = 1;
  CHECK (acm_rules_matrix (row_ptr, col, val, n_texts, 4, terms, rule_ptr, need, n_rules, fired_ptr, fired, 14, &n_fired) == ACM_GPU_E_ARG);
  row_ptr[0] = 0;
  col[6] = 4;
  CHECK (acm_rules_matrix (row_ptr, col, val, n_texts, 4, terms, rule_ptr, need, n_rules, fired_ptr, fired, 14, &n_fired) == ACM_GPU_E_ARG);
  col[6] = 3;
  rule_ptr[1] = 0;
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 4) == ACM_GPU_E_ARG);
  rule_ptr[1] = 2;
  need[0] = 0;
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 4) == ACM_GPU_E_ARG);
  need[0] = 3;
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 4) == ACM_GPU_E_ARG);
  need[0] = 2;
  terms[7].lo = 3;
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 4) == ACM_GPU_E_ARG);
  terms[7].lo = 2;
  rule_ptr[0] = 1;
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 4) == ACM_GPU_E_ARG);
  rule_ptr[0] = 0;
  CHECK (acm_rules_check (terms, rule_ptr, need, n_rules, 4) == ACM_GPU_OK);
  /* what acm_rules runs on the host: the loop, the count matrix in a room of the call's own, the evaluation above */
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
  n_fired = 99;
  memset (fired_ptr, 0xFF, (n_texts + 1) * sizeof *fired_ptr);
  memset (fired, 0xFF, 14 * sizeof *fired);
  CHECK (acm_internal_cpu_rules (m, text, off, n_texts, 3, terms, rule_ptr, need, n_rules, fired_ptr, fired, 14, &n_fired, &total) == ACM_GPU_OK);
  CHECK (n_fired == 14 && total == 10 && memcmp (fired_ptr, want_ptr, sizeof want_ptr) == 0 && memcmp (fired, want, sizeof want) == 0);
  memset (small, '.', 13 * sizeof *small);
  CHECK (acm_internal_cpu_rules (m, text, off, n_texts, 3, terms, rule_ptr, need, n_rules, fired_ptr, small, 13, &n_fired, NULL) == ACM_GPU_E_OVERFLOW);
  CHECK (n_fired == 14 && memcmp (fired_ptr, want_ptr, sizeof want_ptr) == 0);
  for (size_t i = 0; i < 13 * sizeof *small; i++)
    CHECK (((unsigned char *)small)[i] == '.');
  /* 1,500 texts "s he": 3,000 entries, more than the 1,024 the matrix room starts with, so it is grown */
  const uint64_t many = 1500;
  unsigned char *long_text = malloc (3 * 4 * many);
  uint64_t *long_off = malloc ((many + 1) * sizeof *long_off), *long_ptr = malloc ((many + 1) * sizeof *long_ptr);
  uint32_t *long_fired = malloc (4 * many * sizeof *long_fired);
  CHECK (long_text && long_off && long_ptr && long_fired);
  for (uint64_t t = 0; t < many; t++) {
    sym3 (long_text + 12 * t, "s he", 4);
    long_off[t] = 4 * t;
  }
  long_off[many] = 4 * many;
  CHECK (acm_internal_cpu_rules (m, long_text, long_off, many, 3, terms, rule_ptr, need, n_rules, long_ptr, long_fired, 4 * many, &n_fired, &total) ==
         ACM_GPU_OK);
  CHECK (n_fired == 0 * many && total == 2 * many); /* he, s x 1: none of the seven rules */
  const ACMRuleTerm *he_and_s = exact ((ACMRuleTerm[]){ { 0, 1, NO_MAX }, { 3, 1, 1 } }, 2 * sizeof (ACMRuleTerm));
  uint64_t *two_ptr = exact ((uint64_t[]){ 0, 2 }, 2 * sizeof (uint64_t));
  uint32_t *two_need = exact ((uint32_t[]){ 2 }, sizeof (uint32_t));
  CHECK (acm_internal_cpu_rules (m, long_text, long_off, many, 3, he_and_s, two_ptr, two_need, 1, long_ptr, long_fired, many, &n_fired, &total) == ACM_GPU_OK);
  CHECK (n_fired == many && long_ptr[many] == many && long_fired[many - 1] == 0);
  free (two_need), free (two_ptr), free ((void *)he_and_s), free (long_fired), free (long_ptr), free (long_off), free (long_text);
  free (text), free (off);
  acm_release (m);
  for (int k = 0; k < 4; k++)
    free (letters[k]);
  free (big_fired), free (big_fired_ptr), free (big_need), free (big_rule_ptr), free (big_terms), free (big_val), free (big_col), free (big_ptr);
  free (one_ptr), free (zero), free (small), free (fired), free (fired_ptr), free (need), free (rule_ptr), free (terms), free (val), free (col),
    free (row_ptr);
  printf ("all checks held\n");
  return 0;
}
