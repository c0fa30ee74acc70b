/* Test-only driver: acm_chains_check and acm_chains_records (acm_host.c, no HIP) under AddressSanitizer and
 * UBSan.  Every buffer is allocated at its exact size, so that a byte read or written beside it is seen.  The
 * records are made here by a naive loop over the text (every occurrence of every word, by end, longest first:
 * the canonical order), and the join is checked against a naive matcher written here: a recursion over the
 * text itself that tries every gap.  Built and run by tests/test_chains_sanitized.py; exits 0 when every check
 * held. */
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

static const char *const WORDS[] = { "ab", "c", "bc", "a" };
enum { N_WORDS = 4 };
/* ab .{0,2} c;  a .{1,3} a .{0,1} c;  bc alone;  ab then c at once;  a .{2,2} bc */
static const ACMChainTerm TERMS[] = { { 0, 0, 0 }, { 1, 0, 2 }, { 3, 0, 0 }, { 3, 1, 3 }, { 1, 0, 1 }, { 2, 0, 0 },
                                      { 0, 0, 0 }, { 1, 0, 0 }, { 3, 0, 0 }, { 2, 2, 2 } };
static const uint64_t CHAIN_PTR[] = { 0, 2, 5, 6, 8, 10 };
enum { N_CHAINS = 5, N_TERMS = 10 };

/* the greatest start of an embedding of the terms [first, j] whose term j ends at e, inside [lo, ...): -1 for none */
static long
latest_start (const char *text, long lo, const ACMChainTerm *terms, long first, long j, long e) {
  const char *w = WORDS[terms[j].keyword_id];
  const long len = (long)strlen (w), s = e + 1 - len;
  if (s < lo || memcmp (text + s, w, (size_t)len) != 0)
    return -1;
  if (j == first)
    return s;
  long best = -1;
  for (long gap = terms[j].gap_min; gap <= (long)terms[j].gap_max; gap++) {
    const long got = s - 1 - gap >= lo ? latest_start (text, lo, terms, first, j - 1, s - 1 - gap) : -1;
    best = got > best ? got : best;
  }
  return best;
}

/* CHAINS from the text alone, in the total order */
static uint64_t
naive_chains (const char *text, size_t n, const uint64_t *off, uint64_t n_texts, uint64_t pos_base, ACMRecord *out) {
  uint64_t k = 0;
  const uint64_t whole[2] = { 0, n };
  if (!off) {
    off = whole;
    n_texts = 1;
  }
  for (size_t e = 0; e < n; e++)
    for (size_t len = n; len >= 1; len--)
      for (int c = 0; c < N_CHAINS; c++)
        for (uint64_t t = 0; t < n_texts; t++)
          if (off[t] <= e && e < off[t + 1]) {
            const long S = latest_start (text, (long)off[t], TERMS, (long)CHAIN_PTR[c], (long)CHAIN_PTR[c + 1] - 1, (long)e);
            if (S >= 0 && e + 1 - (size_t)S == len)
              out[k++] = (ACMRecord){ pos_base + e, (uint32_t)len, (uint32_t)c };
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

static void
check_errors (void) {
  ACMChainTerm *terms = exact (TERMS, sizeof TERMS);
  uint64_t *ptr = exact (CHAIN_PTR, sizeof CHAIN_PTR);
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_OK);
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS - 1) == ACM_GPU_E_ARG); /* keyword 3 */
  CHECK (acm_chains_check (terms, NULL, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  CHECK (acm_chains_check (NULL, ptr, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  CHECK (acm_chains_check (terms, ptr, 1ull << 31, N_WORDS) == ACM_GPU_E_ARG); /* (refused before ptr is read that far) */
  uint64_t one = 0;
  CHECK (acm_chains_check (NULL, &one, 0, 0) == ACM_GPU_OK); /* no chain */
  ptr[3] = ptr[2];                                           /* a chain without terms */
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[3] = 1; /* decreasing */
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[3] = CHAIN_PTR[3];
  ptr[0] = 1;
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[0] = 0;
  terms[1].gap_min = 3; /* above gap_max */
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  terms[1].gap_min = 0;
  terms[1].gap_max = ACM_CHAIN_GAP_MAX;
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_OK);
  terms[1].gap_max = ACM_CHAIN_GAP_MAX + 1;
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  terms[1].gap_max = 2;
  terms[2].gap_max = 1; /* a first term with a gap */
  CHECK (acm_chains_check (terms, ptr, N_CHAINS, N_WORDS) == ACM_GPU_E_ARG);
  terms[2].gap_max = 0;
  uint64_t far[2] = { 0, 1ull << 31 }; /* refused before terms[] is read */
  CHECK (acm_chains_check (terms, far, 1, N_WORDS) == ACM_GPU_E_ARG);
  far[1] = ACM_CHAIN_TERMS_MAX + 1;
  CHECK (acm_chains_check (terms, far, 1, N_WORDS) == ACM_GPU_E_ARG);
  free (ptr);
  free (terms);
}

/* the join against the naive matcher over `text` cut at off[] (NULL: one text), at pos_base; then the overflow, the
 * count-only and the refused calls */
static uint64_t
check_join (const char *text, const uint64_t *off_in, uint64_t n_texts, uint64_t pos_base) {
  const size_t n = strlen (text);
  ACMChainTerm *terms = exact (TERMS, sizeof TERMS);
  uint64_t *ptr = exact (CHAIN_PTR, sizeof CHAIN_PTR);
  uint64_t *off = off_in ? exact (off_in, (n_texts + 1) * sizeof *off) : NULL;
  uint64_t n_rec = 0, found = 0;
  ACMRecord *rec = naive_records (text, n, WORDS, N_WORDS, pos_base, &n_rec);
  ACMRecord *most = malloc ((n * N_CHAINS + 1) * sizeof *most);
  CHECK (most);
  const uint64_t want_n = naive_chains (text, n, off, n_texts, pos_base, most);
  ACMRecord *want = exact (most, want_n * sizeof *most);
  free (most);
  /* count only */
  CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, NULL, 0, &found) == ACM_GPU_OK);
  CHECK (found == want_n);
  /* the exact room */
  ACMRecord *out = malloc ((want_n ? want_n : 1) * sizeof *out);
  CHECK (out);
  found = 0;
  CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_OK);
  CHECK (found == want_n && same_records (out, want, want_n));
  /* one short: nothing is written (the room of want_n - 1 records is exact: a store would be seen) */
  if (want_n) {
    ACMRecord *tight = malloc ((want_n - 1 ? want_n - 1 : 1) * sizeof *tight);
    CHECK (tight);
    memset (tight, 0x5A, (want_n - 1 ? want_n - 1 : 1) * sizeof *tight);
    found = 0;
    CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, tight, want_n - 1, &found) == ACM_GPU_E_OVERFLOW);
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
    CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    rec[n_rec - 1].length = (uint32_t)n + 1;
    CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1].length = 0;
    CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    if (pos_base)
      CHECK (acm_chains_records (rec, n_rec, n, pos_base + n, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
    if (off && n_texts >= 2 && off[1] < n) {
      const uint64_t cut = off[1];
      off[1] = n + 1;
      CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
      off[1] = cut;
      off[n_texts] = n - 1;
      CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
      off[n_texts] = n;
      off[0] = 1;
      CHECK (acm_chains_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, N_CHAINS, N_WORDS, out, want_n, &found) == ACM_GPU_E_ARG);
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

/* a chain of 16 terms over `a` with gaps 0 to 300 on 400 x `a`: every window holds hundreds of records; the shortest
 * match that ends at e is 16 adjacent symbols */
static void
check_wide (void) {
  enum { A = 400, M = ACM_CHAIN_TERMS_MAX };
  char text[A + 1];
  memset (text, 'a', A);
  text[A] = 0;
  static const char *const words[] = { "a" };
  uint64_t n_rec = 0, found = 0;
  ACMRecord *rec = naive_records (text, A, words, 1, 0, &n_rec);
  CHECK (n_rec == A);
  ACMChainTerm *terms = malloc (M * sizeof *terms);
  CHECK (terms);
  for (uint32_t j = 0; j < M; j++)
    terms[j] = (ACMChainTerm){ 0, 0, j ? 300 : 0 };
  const uint64_t ptr[2] = { 0, M };
  ACMRecord *out = malloc (A * sizeof *out);
  CHECK (out);
  CHECK (acm_chains_records (rec, n_rec, A, 0, NULL, 0, terms, ptr, 1, 1, out, A, &found) == ACM_GPU_OK);
  CHECK (found == A - M + 1);
  for (uint64_t j = 0; j < found; j++)
    CHECK (out[j].end_pos == M - 1 + j && out[j].length == M && out[j].keyword_id == 0);
  /* no record at all, and no symbol at all */
  CHECK (acm_chains_records (NULL, 0, A, 0, NULL, 0, terms, ptr, 1, 1, out, A, &found) == ACM_GPU_OK && found == 0);
  const uint64_t none[1] = { 0 };
  CHECK (acm_chains_records (NULL, 0, 0, 0, none, 0, terms, ptr, 1, 1, NULL, 0, &found) == ACM_GPU_OK && found == 0);
  CHECK (acm_chains_records (rec, n_rec, A, 0, NULL, 0, terms, ptr, 1, 1, out, A, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_chains_records (rec, n_rec, A, 0, NULL, 0, terms, ptr, 1, 1, NULL, A, &found) == ACM_GPU_E_ARG);
  free (out);
  free (terms);
  free (rec);
}

int
main (void) {
  check_errors ();
  uint64_t matches = 0;
  const char *text = "abc ab.c a.a.c abxxc bc aabcc a..bc";
  matches += check_join (text, NULL, 0, 0);
  matches += check_join (text, NULL, 0, 1ull << 40);
  const uint64_t cuts[] = { 0, 0, 2, 9, 9, 12, 19, 35, 35 }; /* empty texts, a cut inside `abc` and one inside `a.a.c` */
  matches += check_join (text, cuts, 8, 0);
  matches += check_join (text, cuts, 8, 77);
  matches += check_join ("", NULL, 0, 0);
  matches += check_join ("zzzz", NULL, 0, 0);
  CHECK (matches > 40);
  check_wide ();
  printf ("all checks held (%llu matches)\n", (unsigned long long)matches);
  return 0;
}
