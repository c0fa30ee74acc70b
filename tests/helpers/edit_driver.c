/* Test-only driver: acm_edit_check and acm_edit_records (acm_host.c, no HIP) under AddressSanitizer and UBSan.
 * Every buffer is allocated at its exact size, so that a byte read or written beside it is seen.  The target of a
 * case is cut here by the canonical cut, the records are made here by a naive loop over the text (every occurrence
 * of every piece, by end, longest first: the canonical order), and the result is checked against a naive scan
 * written here: for every end and every start a plain Levenshtein distance, the largest start among the best.
 * Built and run by tests/test_edit_sanitized.py; exits 0 when every check held. */
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

/* a copy at the exact size (one byte for nothing) */
static void *
exact (const void *from, size_t bytes) {
  void *to = malloc (bytes ? bytes : 1);
  CHECK (to);
  if (bytes)
    memcpy (to, from, bytes);
  return to;
}

enum { MOST_PIECES = 16, MOST = 64 };

/* one target with its canonical cut; the distinct pieces are the keywords, in order of first appearance */
struct set {
  char *spell;
  uint64_t *spell_off, *tgt_ptr;
  uint32_t *k;
  ACMPatternTerm *terms;
  char words[MOST_PIECES][MOST];
  int n_words;
  uint64_t n_terms, L;
};

static void
make_set (struct set *s, const char *target, uint32_t k) {
  const uint64_t L = strlen (target), spell_off[2] = { 0, L };
  ACMPatternTerm terms[MOST_PIECES];
  s->n_words = 0;
  s->n_terms = 0;
  s->L = L;
  for (uint32_t j = 0; j <= k; j++) {
    uint64_t b = 0, e = 0;
    CHECK (acm_approx_split (L, k, j, &b, &e) == ACM_GPU_OK);
    char piece[MOST] = { 0 };
    memcpy (piece, target + b, e - b);
    int id = 0;
    while (id < s->n_words && strcmp (s->words[id], piece))
      id++;
    if (id == s->n_words)
      strcpy (s->words[s->n_words++], piece);
    terms[s->n_terms++] = (ACMPatternTerm){ (uint32_t)id, (uint32_t)b, (uint32_t)(e - b) };
  }
  const uint64_t tgt_ptr[2] = { 0, s->n_terms };
  s->spell = exact (target, L);
  s->spell_off = exact (spell_off, sizeof spell_off);
  s->tgt_ptr = exact (tgt_ptr, sizeof tgt_ptr);
  s->k = exact (&k, sizeof k);
  s->terms = exact (terms, s->n_terms * sizeof *terms);
}

static void
free_set (struct set *s) {
  free (s->spell);
  free (s->spell_off);
  free (s->tgt_ptr);
  free (s->k);
  free (s->terms);
}

/* every occurrence of every word in text[0 .. n), by end ascending, longest first */
static ACMRecord *
naive_records (const char *text, size_t n, const struct set *s, uint64_t pos_base, uint64_t *found) {
  uint64_t k = 0;
  ACMRecord *tmp = malloc ((n * (size_t)s->n_words + 1) * sizeof *tmp);
  CHECK (tmp);
  for (size_t e = 0; e < n; e++)
    for (size_t len = MOST - 1; len >= 1; len--)
      for (int w = 0; w < s->n_words; w++)
        if (strlen (s->words[w]) == len && len <= e + 1 && memcmp (text + e + 1 - len, s->words[w], len) == 0)
          tmp[k++] = (ACMRecord){ pos_base + e, (uint32_t)len, (uint32_t)w };
  ACMRecord *out = exact (tmp, k * sizeof *tmp);
  free (tmp);
  *found = k;
  return out;
}

/* the unit-cost Levenshtein distance of a[0 .. la) and b[0 .. lb) */
static uint32_t
naive_ed (const char *a, size_t la, const char *b, size_t lb) {
  uint32_t prev[2 * MOST], cur[2 * MOST];
  CHECK (lb < 2 * MOST);
  for (size_t j = 0; j <= lb; j++)
    prev[j] = (uint32_t)j;
  for (size_t i = 1; i <= la; i++) {
    cur[0] = (uint32_t)i;
    for (size_t j = 1; j <= lb; j++) {
      uint32_t v = prev[j - 1] + (a[i - 1] != b[j - 1]);
      if (prev[j] + 1 < v)
        v = prev[j] + 1;
      if (cur[j - 1] + 1 < v)
        v = cur[j - 1] + 1;
      cur[j] = v;
    }
    memcpy (prev, cur, (lb + 1) * sizeof *cur);
  }
  return prev[lb];
}

/* every end of every text at which the target is within its budget: the least distance over all starts of that text and the
 * largest start that attains it */
static uint64_t
naive_edit (const char *text, size_t n, const uint64_t *off, uint64_t n_texts, uint64_t pos_base, const struct set *s, ACMRecord *out, uint32_t *dist) {
  uint64_t found = 0;
  const uint64_t whole[2] = { 0, n };
  if (!off) {
    off = whole;
    n_texts = 1;
  }
  for (uint64_t t = 0; t < n_texts; t++)
    for (uint64_t e = off[t]; e < off[t + 1]; e++) {
      uint32_t best = UINT32_MAX;
      uint64_t best_s = 0;
      for (uint64_t st = off[t]; st <= e + 1; st++) {
        if (e + 1 - st >= 2 * MOST)
          continue; /* (much longer than the target and its budget) */
        const uint32_t d = naive_ed (s->spell, s->L, text + st, e + 1 - st);
        if (d <= best) {
          best = d;
          best_s = st;
        }
      }
      if (best <= s->k[0]) {
        out[found] = (ACMRecord){ pos_base + e, (uint32_t)(e + 1 - best_s), 0 };
        dist[found++] = best;
      }
    }
  return found;
}

/* acm_edit_records on exact-size buffers against the naive scan; returns the number of matches */
static uint64_t
one_case (const char *target, uint32_t k, const char *text_z, const uint64_t *off_in, uint64_t n_texts, uint64_t pos_base) {
  struct set s;
  make_set (&s, target, k);
  const size_t n = strlen (text_z);
  char *text = exact (text_z, n);
  uint64_t *off = off_in ? exact (off_in, (n_texts + 1) * sizeof *off) : NULL;
  uint64_t n_rec = 0, found = 0, counted = 0;
  ACMRecord *rec = naive_records (text, n, &s, pos_base, &n_rec);
  CHECK (acm_edit_check (s.spell_off, s.k, s.terms, s.tgt_ptr, 1, (uint64_t)s.n_words) == ACM_GPU_OK);
  ACMRecord *want = malloc ((n + 1) * sizeof *want);
  uint32_t *want_d = malloc ((n + 1) * sizeof *want_d);
  CHECK (want && want_d);
  const uint64_t total = naive_edit (text, n, off, n_texts, pos_base, &s, want, want_d);
  CHECK (acm_edit_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, s.spell, s.spell_off, s.k, s.terms, s.tgt_ptr, 1, (uint64_t)s.n_words, NULL,
                           NULL, 0, &counted) == ACM_GPU_OK);
  CHECK (counted == total);
  ACMRecord *out = malloc ((total ? total : 1) * sizeof *out);
  uint32_t *dist = malloc ((total ? total : 1) * sizeof *dist);
  CHECK (out && dist);
  CHECK (acm_edit_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, s.spell, s.spell_off, s.k, s.terms, s.tgt_ptr, 1, (uint64_t)s.n_words, out,
                           dist, total, &found) == ACM_GPU_OK);
  CHECK (found == total);
  for (uint64_t i = 0; i < total; i++)
    CHECK (out[i].end_pos == want[i].end_pos && out[i].length == want[i].length && out[i].keyword_id == 0 && dist[i] == want_d[i]);
  if (total) { /* one entry too few: the count that suffices, nothing written (the buffers are one entry short) */
    ACMRecord *few = malloc ((total - 1 ? total - 1 : 1) * sizeof *few);
    uint32_t *few_d = malloc ((total - 1 ? total - 1 : 1) * sizeof *few_d);
    CHECK (few && few_d);
    found = 0;
    CHECK (acm_edit_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, s.spell, s.spell_off, s.k, s.terms, s.tgt_ptr, 1, (uint64_t)s.n_words,
                             total - 1 ? few : NULL, few_d, total - 1, &found) == (total - 1 ? ACM_GPU_E_OVERFLOW : ACM_GPU_OK));
    CHECK (found == total);
    free (few);
    free (few_d);
  }
  free (out);
  free (dist);
  free (want);
  free (want_d);
  free (rec);
  free (off);
  free (text);
  free_set (&s);
  return total;
}

static void
named_cases (void) {
  /* one deletion, one insertion, one substitution; the first and the last symbol */
  CHECK (one_case ("Dalloway", 1, "Mrs Daloway said", NULL, 0, 0) >= 1);
  CHECK (one_case ("Dalloway", 1, "Mrs Dallloway said", NULL, 0, 0) >= 1);
  CHECK (one_case ("Dalloway", 1, "Mrs Dalloxay said", NULL, 0, 0) >= 1);
  CHECK (one_case ("Dalloway", 1, "alloway", NULL, 0, 0) >= 1);
  CHECK (one_case ("Dalloway", 1, "Dallowa", NULL, 0, 0) >= 1);
  CHECK (one_case ("Dalloway", 1, "Mrs Dalloway said", NULL, 0, 1ull << 40) == 3);
  /* a transposition costs 2 */
  CHECK (one_case ("Dalloway", 1, "Mrs Dalolway said", NULL, 0, 0) == 0);
  CHECK (one_case ("Dalloway", 2, "Mrs Dalolway said", NULL, 0, 0) >= 1);
  /* a periodic text and two identical pieces: many seeds per end */
  CHECK (one_case ("abab", 1, "abababab", NULL, 0, 0) == 6);
  CHECK (one_case ("abab", 1, "ab", NULL, 0, 0) == 0);
  CHECK (one_case ("abab", 3, "b", NULL, 0, 0) == 1);
  /* a text that ends inside a target, one that begins inside it; the band clipped at both ends of the buffer */
  CHECK (one_case ("Dalloway", 2, "said Dallow", NULL, 0, 0) >= 1);
  CHECK (one_case ("Dalloway", 2, "lloway said", NULL, 0, 0) >= 1);
  CHECK (one_case ("Dalloway", 3, "Dalloway", NULL, 0, 0) >= 4);
  CHECK (one_case ("abcdefghijklmnopqrstuvwxyzABCDEF", 15, "xxabcdefhijklmnopqrstuvwxyzABCDEFxx", NULL, 0, 0) >= 1);
  /* k = 0: the exact occurrences */
  CHECK (one_case ("the", 0, "the cat sat on the mat; the end", NULL, 0, 0) == 3);
  /* texts: a cut inside the word, empty texts, no text at all */
  const uint64_t cut[] = { 0, 8, 17 }, empties[] = { 0, 0, 9, 9, 17, 17 }, none[] = { 0 };
  CHECK (one_case ("Dalloway", 1, "Mrs Dalloway said", cut, 2, 0) == 0);
  CHECK (one_case ("Dalloway", 3, "Mrs Dalloway said", empties, 5, 7) >= 1);
  CHECK (one_case ("Dalloway", 1, "", none, 0, 0) == 0);
  CHECK (one_case ("Dalloway", 1, "", NULL, 0, 0) == 0);
}

static void
refused_inputs (void) {
  struct set s;
  make_set (&s, "Dalloway", 1);
  const char *text_z = "Mrs Dalloway said";
  const size_t n = strlen (text_z);
  char *text = exact (text_z, n);
  uint64_t n_rec = 0, found = 77;
  ACMRecord *rec = naive_records (text, n, &s, 0, &n_rec);
  ACMRecord out[8];
  uint32_t dist[8];
  memset (out, 0x55, sizeof out);
  memset (dist, 0x55, sizeof dist);
  CHECK (n_rec == 2);
#define CALL(records, n_symbols, pos_base, off, n_texts, kk, nk)                                                                                        \
  acm_edit_records (records, n_rec, text, 1, n_symbols, pos_base, off, n_texts, s.spell, s.spell_off, kk, s.terms, s.tgt_ptr, 1, nk, out, dist, 8, &found)
  /* the two conditions of the edit calls; acm_approx_check takes the same arguments */
  uint32_t *k16 = exact (&(uint32_t){ 16 }, 4), *k8 = exact (&(uint32_t){ 8 }, 4), *k7 = exact (&(uint32_t){ 7 }, 4);
  CHECK (acm_edit_check (s.spell_off, k8, s.terms, s.tgt_ptr, 1, 2) == ACM_GPU_E_ARG && acm_approx_check (s.spell_off, k8, s.terms, s.tgt_ptr, 1, 2) == 0);
  CHECK (acm_edit_check (s.spell_off, k16, s.terms, s.tgt_ptr, 1, 2) == ACM_GPU_E_ARG && acm_approx_check (s.spell_off, k16, s.terms, s.tgt_ptr, 1, 2) == 0);
  CHECK (acm_edit_check (s.spell_off, k7, s.terms, s.tgt_ptr, 1, 2) == ACM_GPU_OK);
  CHECK (acm_edit_check (s.spell_off, s.k, s.terms, s.tgt_ptr, 1, 1) == ACM_GPU_E_ARG); /* keyword_id >= n_keywords */
  CHECK (acm_edit_check (NULL, NULL, NULL, NULL, 0, 0) == ACM_GPU_E_ARG);
  CHECK (CALL (rec, n, 0, NULL, 0, k8, 2) == ACM_GPU_E_ARG);
  CHECK (CALL (rec, n, 0, NULL, 0, s.k, 1) == ACM_GPU_E_ARG);
  /* records outside the buffer, of length 0; offsets that break the contract */
  CHECK (CALL (rec, rec[1].end_pos, 0, NULL, 0, s.k, 2) == ACM_GPU_E_ARG);
  CHECK (CALL (rec, n, rec[0].end_pos, NULL, 0, s.k, 2) == ACM_GPU_E_ARG);
  ACMRecord *zero = exact (rec, n_rec * sizeof *rec);
  zero[1].length = 0;
  CHECK (CALL (zero, n, 0, NULL, 0, s.k, 2) == ACM_GPU_E_ARG);
  const uint64_t down[] = { 0, 10, 5, 17 }, late[] = { 1, 17 }, early[] = { 0, 16 };
  CHECK (CALL (rec, n, 0, down, 3, s.k, 2) == ACM_GPU_E_ARG);
  CHECK (CALL (rec, n, 0, late, 1, s.k, 2) == ACM_GPU_E_ARG);
  CHECK (CALL (rec, n, 0, early, 1, s.k, 2) == ACM_GPU_E_ARG);
  for (size_t i = 0; i < sizeof out; i++)
    CHECK (((unsigned char *)out)[i] == 0x55);
  for (size_t i = 0; i < sizeof dist; i++)
    CHECK (((unsigned char *)dist)[i] == 0x55);
  /* records that are not in canonical order, and a keyword the set does not know: an unspecified result, nothing out of bounds */
  ACMRecord *swapped = exact (rec, n_rec * sizeof *rec);
  swapped[0] = rec[1];
  swapped[1] = rec[0];
  swapped[0].keyword_id = 9;
  CHECK (CALL (swapped, n, 0, NULL, 0, s.k, 2) == ACM_GPU_OK);
  CHECK (CALL (rec, n, 0, NULL, 0, s.k, 2) == ACM_GPU_OK && found == 3);
#undef CALL
  free (swapped);
  free (zero);
  free (k16);
  free (k8);
  free (k7);
  free (rec);
  free (text);
  free_set (&s);
}

int
main (void) {
  named_cases ();
  refused_inputs ();
  printf ("all checks held\n");
  return 0;
}
