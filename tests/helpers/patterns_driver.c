/* Test-only driver: acm_patterns_check and acm_patterns_records (acm_host.c, no HIP) under AddressSanitizer
 * and UBSan.  Every buffer is allocated at its exact size, so that a byte read or written beside it is
 * seen.  The records are made here by a naive loop over the text (every occurrence of every fragment, by end,
 * longest first: the canonical order), and the join is checked against a naive template matcher written
 * here.  Built and run by tests/test_patterns_sanitized.py; exits 0 when every check held. */
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

/* every occurrence of every word in text[0 .. n), by end ascending, longest first */
static ACMRecord *
naive_records (const char *text, size_t n, const char *const *words, int n_words, uint64_t pos_base, uint64_t *found) {
  uint64_t k = 0;
  ACMRecord *tmp = malloc ((n * (size_t)n_words + 1) * sizeof *tmp);
  CHECK (tmp);
  for (size_t e = 0; e < n; e++)
    for (size_t len = n; len >= 1; len--)
      for (int w = 0; w < n_words; w++)
        if (strlen (words[w]) == len && len <= e + 1 && memcmp (text + e + 1 - len, words[w], len) == 0)
          tmp[k++] = (ACMRecord){ pos_base + e, (uint32_t)len, (uint32_t)w };
  ACMRecord *out = exact (tmp, k * sizeof *tmp);
  free (tmp);
  *found = k;
  return out;
}

/* every occurrence of every template ('?' matches any one symbol) inside one text, by end ascending, longest first,
 * template ascending */
static uint64_t
naive_templates (const char *text, size_t n, const uint64_t *off, uint64_t n_texts, const char *const *tpl, int n_tpl, uint64_t pos_base,
                 ACMRecord *out) {
  uint64_t k = 0;
  const uint64_t whole[2] = { 0, n };
  if (!off) {
    off = whole;
    n_texts = 1;
  }
  for (size_t e = 0; e < n; e++)
    for (size_t len = n; len >= 1; len--)
      for (int p = 0; p < n_tpl; p++) {
        if (strlen (tpl[p]) != len || len > e + 1)
          continue;
        const size_t s = e + 1 - len;
        int inside = 0, same = 1;
        for (uint64_t t = 0; t < n_texts; t++)
          inside = inside || (off[t] <= s && e < off[t + 1]);
        for (size_t i = 0; i < len; i++)
          same = same && (tpl[p][i] == '?' || tpl[p][i] == text[s + i]);
        if (inside && same)
          out[k++] = (ACMRecord){ pos_base + e, (uint32_t)len, (uint32_t)p };
      }
  return k;
}

static int
same_records (const ACMRecord *a, const ACMRecord *b, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (a[i].end_pos != b[i].end_pos || a[i].length != b[i].length || a[i].keyword_id != b[i].keyword_id)
      return 0;
  return 1;
}

/* fragments of the templates below */
static const char *const WORDS[] = { "ab", "d", "cd", "a", "bc", "c" };
enum { N_WORDS = 6 };
/* a?c?, ab?d, a?cd, ?bc, ab (no don't-care), a??d with its terms the other way round */
static const char *const TEMPLATES[] = { "a?c", "ab?d", "a?cd", "?bc", "ab", "a??d" };
static const ACMPatternTerm TERMS[] = { { 3, 0, 1 }, { 5, 2, 1 }, { 0, 0, 2 }, { 1, 3, 1 }, { 3, 0, 1 }, { 2, 2, 2 }, { 4, 1, 2 },
                                        { 0, 0, 2 }, { 1, 3, 1 }, { 3, 0, 1 } };
static const uint64_t PAT_PTR[] = { 0, 2, 4, 6, 7, 8, 10 };
enum { N_PATTERNS = 6, N_TERMS = 10 };

static void
check_errors (void) {
  ACMPatternTerm *terms = exact (TERMS, sizeof TERMS);
  uint64_t *ptr = exact (PAT_PTR, sizeof PAT_PTR);
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_OK);
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS - 1) == ACM_GPU_E_ARG); /* keyword 5 */
  CHECK (acm_patterns_check (terms, NULL, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  CHECK (acm_patterns_check (NULL, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  CHECK (acm_patterns_check (terms, ptr, 1ull << 31, N_WORDS) == ACM_GPU_E_ARG); /* (refused before ptr is read that far) */
  uint64_t one = 0;
  CHECK (acm_patterns_check (NULL, &one, 0, 0) == ACM_GPU_OK); /* no pattern */
  ptr[3] = ptr[2]; /* a pattern without terms */
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[3] = 1; /* decreasing */
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[3] = PAT_PTR[3];
  ptr[0] = 1;
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[0] = 0;
  terms[4].length = 0;
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  terms[4].length = 0xFFFFFFFFu; /* offset + length wraps in 32 bits */
  terms[4].offset = 2;
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  terms[4].length = 1;
  terms[4].offset = (1u << 31) - 1;
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_E_ARG);
  terms[4].offset = (1u << 31) - 2;
  CHECK (acm_patterns_check (terms, ptr, N_PATTERNS, N_WORDS) == ACM_GPU_OK);
  uint64_t far[2] = { 0, 1ull << 31 }; /* 2^31 terms: refused before terms[] is read */
  CHECK (acm_patterns_check (terms, far, 1, N_WORDS) == ACM_GPU_E_ARG);
  free (ptr);
  free (terms);
}

/* the join against the naive matcher over `text` cut at off[] (NULL: one text), at pos_base; then the overflow, the
 * count-only and the refused calls */
static uint64_t
check_join (const char *text, const uint64_t *off_in, uint64_t n_texts, uint64_t pos_base) {
  const size_t n = strlen (text);
  ACMPatternTerm *terms = exact (TERMS, sizeof TERMS);
  uint64_t *ptr = exact (PAT_PTR, sizeof PAT_PTR);
  uint64_t *off = off_in ? exact (off_in, (n_texts + 1) * sizeof *off) : NULL;
  uint64_t n_rec = 0, found = 0;
  ACMRecord *rec = naive_records (text, n, WORDS, N_WORDS, pos_base, &n_rec);
  ACMRecord *most = malloc ((n * N_PATTERNS + 1) * sizeof *most);
  CHECK (most);
  const uint64_t want_n = naive_templates (text, n, off, n_texts, TEMPLATES, N_PATTERNS, pos_base, most);
  ACMRecord *want = exact (most, want_n * sizeof *most);
  free (most);
  /* count only */
  CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, NULL, 0, &found) == ACM_GPU_OK);
  CHECK (found == want_n);
  /* the exact room */
  ACMRecord *out = malloc ((want_n ? want_n : 1) * sizeof *out);
  CHECK (out);
  found = 0;
  CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_OK);
  CHECK (found == want_n && same_records (out, want, want_n));
  /* one short: nothing is written (the room of want_n - 1 records is exact: a store would be seen) */
  if (want_n) {
    ACMRecord *tight = malloc ((want_n - 1 ? want_n - 1 : 1) * sizeof *tight);
    CHECK (tight);
    memset (tight, 0x5A, (want_n - 1 ? want_n - 1 : 1) * sizeof *tight);
    found = 0;
    CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, tight, want_n - 1, &found) == ACM_GPU_E_OVERFLOW);
    CHECK (found == want_n);
    for (size_t b = 0; b < (want_n - 1) * sizeof *tight; b++)
      CHECK (((unsigned char *)tight)[b] == 0x5A);
    free (tight);
  }
  /* refused: a record outside the buffer (its end, its start), of length 0; offsets that break the contract */
  if (n_rec) {
    memset (out, 0x5A, (want_n ? want_n : 1) * sizeof *out);
    const ACMRecord kept = rec[n_rec - 1];
    rec[n_rec - 1].end_pos = pos_base + n;
    CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    rec[n_rec - 1].length = (uint32_t)n + 1;
    CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1].length = 0;
    CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    if (pos_base)
      CHECK (acm_patterns_records (rec, n_rec, n, pos_base + n, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    if (off && n_texts >= 2 && off[1] < n) {
      const uint64_t cut = off[1];
      off[1] = n + 1;
      CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
      off[1] = cut;
      off[n_texts] = n - 1;
      CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
      off[n_texts] = n;
      off[0] = 1;
      CHECK (acm_patterns_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_PATTERNS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
      off[0] = 0;
    }
    for (size_t b = 0; b < want_n * sizeof *out; b++)
      CHECK (((unsigned char *)out)[b] == 0x5A);
  }
  free (out);
  free (want);
  free (rec);
  free (off);
  free (ptr);
  free (terms);
  return want_n;
}

/* `a` followed by k don't-cares and `z`, k = 1 .. 100, on 120 x `a` and a `z`: 100 matches that end at the `z`, each
 * anchored at the same record, plus the terms the other way round for every second pattern */
static void
check_pile (void) {
  enum { A = 120, K = 100 };
  char text[A + 2];
  memset (text, 'a', A);
  text[A] = 'z';
  text[A + 1] = 0;
  static const char *const words[] = { "a", "z" };
  uint64_t n_rec = 0, found = 0;
  ACMRecord *rec = naive_records (text, A + 1, words, 2, 0, &n_rec);
  CHECK (n_rec == A + 1);
  ACMPatternTerm *terms = malloc (2 * K * sizeof *terms);
  uint64_t *ptr = malloc ((K + 1) * sizeof *ptr);
  CHECK (terms && ptr);
  for (uint32_t k = 1; k <= K; k++) {
    const ACMPatternTerm a = { 0, 0, 1 }, z = { 1, k + 1, 1 };
    terms[2 * (k - 1)] = k % 2 ? a : z;
    terms[2 * (k - 1) + 1] = k % 2 ? z : a;
    ptr[k - 1] = 2 * (k - 1);
  }
  ptr[K] = 2 * K;
  ACMRecord *out = malloc (K * sizeof *out);
  CHECK (out);
  CHECK (acm_patterns_records (rec, n_rec, A + 1, 0, NULL, 0, terms, ptr, K, 2, out, K, &found) == ACM_GPU_OK);
  CHECK (found == K);
  for (uint32_t j = 0; j < K; j++) /* the longest first: k = 100 is pattern 99 */
    CHECK (out[j].end_pos == A && out[j].length == K + 2 - j && out[j].keyword_id == K - 1 - j);
  /* no record at all, and no symbol at all */
  CHECK (acm_patterns_records (NULL, 0, A + 1, 0, NULL, 0, terms, ptr, K, 2, out, K, &found) == ACM_GPU_OK && found == 0);
  const uint64_t none[1] = { 0 };
  CHECK (acm_patterns_records (NULL, 0, 0, 0, none, 0, terms, ptr, K, 2, NULL, 0, &found) == ACM_GPU_OK && found == 0);
  CHECK (acm_patterns_records (rec, n_rec, A + 1, 0, NULL, 0, terms, ptr, K, 2, out, K, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_patterns_records (rec, n_rec, A + 1, 0, NULL, 0, terms, ptr, K, 2, NULL, K, &found) == ACM_GPU_E_ARG);
  free (out);
  free (ptr);
  free (terms);
  free (rec);
}

int
main (void) {
  check_errors ();
  uint64_t matches = 0;
  matches += check_join ("abcd abxd axcd xbc ab aabcdd", NULL, 0, 0);
  matches += check_join ("abcd abxd axcd xbc ab aabcdd", NULL, 0, 1ull << 40);
  const uint64_t cuts[] = { 0, 0, 2, 9, 9, 14, 19, 28, 28 }; /* empty texts, a cut inside `abcd`, a template that fills a text */
  matches += check_join ("abcd abxd axcd xbc ab aabcdd", cuts, 8, 0);
  matches += check_join ("abcd abxd axcd xbc ab aabcdd", cuts, 8, 77);
  matches += check_join ("", NULL, 0, 0);
  matches += check_join ("zzzz", NULL, 0, 0);
  CHECK (matches > 40);
  check_pile ();
  printf ("all checks held (%llu matches)\n", (unsigned long long)matches);
  return 0;
}
