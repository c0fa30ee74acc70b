/* Test-only driver: acm_approx_check, acm_approx_split and acm_approx_records (acm_host.c, no HIP) under
 * AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte read or written beside
 * it is seen.  The targets are cut here by the canonical cut, the records are made here by a naive loop over the
 * text (every occurrence of every piece, by end, longest first: the canonical order), and the join is checked
 * against a naive Hamming scan written here.  Built and run by tests/test_approx_sanitized.py; exits 0 when every
 * check held. */
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

static const char *const TARGETS[] = { "abcdefgh", "cdefg", "hab", "ab" };
static const uint32_t BUDGET[] = { 2, 1, 1, 0 };
enum { N_TARGETS = 4, MOST_PIECES = 16 };

/* the set of a run: the distinct pieces are the keywords, in order of first appearance */
struct set {
  char *spell;
  uint64_t *spell_off, *tgt_ptr;
  uint32_t *k;
  ACMPatternTerm *terms;
  char words[MOST_PIECES][16];
  int n_words;
  uint64_t n_terms;
};

static void
make_set (struct set *s) {
  char spell[64];
  uint64_t spell_off[N_TARGETS + 1] = { 0 }, tgt_ptr[N_TARGETS + 1] = { 0 };
  ACMPatternTerm terms[MOST_PIECES];
  s->n_words = 0;
  s->n_terms = 0;
  for (int w = 0; w < N_TARGETS; w++) {
    const uint64_t L = strlen (TARGETS[w]);
    memcpy (spell + spell_off[w], TARGETS[w], L);
    spell_off[w + 1] = spell_off[w] + L;
    for (uint32_t j = 0; j <= BUDGET[w]; j++) {
      uint64_t b = 0, e = 0;
      CHECK (acm_approx_split (L, BUDGET[w], j, &b, &e) == ACM_GPU_OK);
      CHECK (b == j * L / (BUDGET[w] + 1) && e == (j + 1) * L / (BUDGET[w] + 1) && b < e && e <= L);
      char piece[16] = { 0 };
      memcpy (piece, TARGETS[w] + b, e - b);
      int id = 0;
      while (id < s->n_words && strcmp (s->words[id], piece))
        id++;
      if (id == s->n_words)
        strcpy (s->words[s->n_words++], piece);
      terms[s->n_terms++] = (ACMPatternTerm){ (uint32_t)id, (uint32_t)b, (uint32_t)(e - b) };
    }
    tgt_ptr[w + 1] = s->n_terms;
  }
  s->spell = exact (spell, spell_off[N_TARGETS]);
  s->spell_off = exact (spell_off, sizeof spell_off);
  s->tgt_ptr = exact (tgt_ptr, sizeof tgt_ptr);
  s->k = exact (BUDGET, sizeof BUDGET);
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
    for (size_t len = 16; len >= 1; len--)
      for (int w = 0; w < s->n_words; w++)
        if (strlen (s->words[w]) == len && len <= e + 1 && memcmp (text + e + 1 - len, s->words[w], len) == 0)
          tmp[k++] = (ACMRecord){ pos_base + e, (uint32_t)len, (uint32_t)w };
  ACMRecord *out = exact (tmp, k * sizeof *tmp);
  free (tmp);
  *found = k;
  return out;
}

/* every window of every target within its budget inside one text, by end ascending, longest first, target ascending */
static uint64_t
naive_hamming (const char *text, size_t n, const uint64_t *off, uint64_t n_texts, uint64_t pos_base, ACMRecord *out, uint32_t *dist) {
  uint64_t k = 0;
  const uint64_t whole[2] = { 0, n };
  if (!off) {
    off = whole;
    n_texts = 1;
  }
  for (size_t e = 0; e < n; e++)
    for (size_t len = 16; len >= 1; len--)
      for (int w = 0; w < N_TARGETS; w++) {
        if (strlen (TARGETS[w]) != len || len > e + 1)
          continue;
        const size_t s = e + 1 - len;
        int inside = 0;
        uint32_t d = 0;
        for (uint64_t t = 0; t < n_texts; t++)
          inside = inside || (off[t] <= s && e < off[t + 1]);
        for (size_t i = 0; i < len; i++)
          d += TARGETS[w][i] != text[s + i];
        if (inside && d <= BUDGET[w]) {
          out[k] = (ACMRecord){ pos_base + e, (uint32_t)len, (uint32_t)w };
          dist[k++] = d;
        }
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
  struct set s;
  make_set (&s);
  const uint64_t nk = (uint64_t)s.n_words;
  uint64_t b = 0, e = 0;
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_OK);
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk - 1) == ACM_GPU_E_ARG);
  CHECK (acm_approx_check (NULL, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  CHECK (acm_approx_check (s.spell_off, NULL, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  CHECK (acm_approx_check (s.spell_off, s.k, NULL, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, NULL, N_TARGETS, nk) == ACM_GPU_E_ARG);
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, 1ull << 31, nk) == ACM_GPU_E_ARG); /* (refused before the arrays are read that far) */
  uint64_t one = 0;
  CHECK (acm_approx_check (&one, NULL, NULL, &one, 0, 0) == ACM_GPU_OK); /* no target */
  s.tgt_ptr[2] = s.tgt_ptr[1]; /* a target without terms */
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.tgt_ptr[2] = 1; /* decreasing */
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.tgt_ptr[2] = 5;
  s.tgt_ptr[0] = 1;
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.tgt_ptr[0] = 0;
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_OK);
  s.spell_off[2] = s.spell_off[1]; /* L == 0 */
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.spell_off[2] = 13;
  s.spell_off[0] = 1;
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.spell_off[0] = 0;
  s.k[3] = 256;
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.k[3] = 255; /* (the check knows no cut: a budget above the number of terms is no error) */
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_OK);
  s.terms[4].length = 0;
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.terms[4].length = 0xFFFFFFFFu; /* offset + length wraps in 32 bits */
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.terms[4].length = 4; /* `cdefg` is 5 symbols long: a piece at 2 of 4 symbols ends behind it */
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_E_ARG);
  s.terms[4].length = 3;
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk) == ACM_GPU_OK);
  uint64_t far[2] = { 0, 1ull << 31 }; /* 2^31 terms: refused before terms[] is read */
  CHECK (acm_approx_check (s.spell_off, s.k, s.terms, far, 1, nk) == ACM_GPU_E_ARG);
  CHECK (acm_approx_split (4, 3, 3, &b, &e) == ACM_GPU_OK && b == 3 && e == 4); /* L == k + 1 */
  CHECK (acm_approx_split (3, 3, 0, &b, &e) == ACM_GPU_E_ARG);                  /* L < k + 1 */
  CHECK (acm_approx_split (8, 1, 2, &b, &e) == ACM_GPU_E_ARG);
  CHECK (acm_approx_split (8, 1, 0, NULL, &e) == ACM_GPU_E_ARG && acm_approx_split (8, 1, 0, &b, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_approx_split ((1ull << 31) - 1, 255, 255, &b, &e) == ACM_GPU_OK && e == (1ull << 31) - 1);
  CHECK (acm_approx_split (1ull << 31, 0, 0, &b, &e) == ACM_GPU_E_ARG);
  free_set (&s);
}

/* the join against the naive scan over `text` cut at off[] (NULL: one text), at pos_base; then the overflow, the
 * count-only and the refused calls */
static uint64_t
check_join (const char *text_in, const uint64_t *off_in, uint64_t n_texts, uint64_t pos_base) {
  const size_t n = strlen (text_in);
  struct set s;
  make_set (&s);
  const uint64_t nk = (uint64_t)s.n_words;
  char *text = exact (text_in, n);
  uint64_t *off = off_in ? exact (off_in, (n_texts + 1) * sizeof *off) : NULL;
  uint64_t n_rec = 0, found = 0;
  ACMRecord *rec = naive_records (text, n, &s, pos_base, &n_rec);
  ACMRecord *most = malloc ((n * N_TARGETS + 1) * sizeof *most);
  uint32_t *most_d = malloc ((n * N_TARGETS + 1) * sizeof *most_d);
  CHECK (most && most_d);
  const uint64_t want_n = naive_hamming (text, n, off, n_texts, pos_base, most, most_d);
  ACMRecord *want = exact (most, want_n * sizeof *most);
  uint32_t *want_d = exact (most_d, want_n * sizeof *most_d);
  free (most);
  free (most_d);
#define APPROX(records, n_symbols, base, offsets, out, dist, cap)                                                                          \
  acm_approx_records (records, n_rec, text, 1, n_symbols, base, offsets, n_texts, s.spell, s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk, out, dist, \
                      cap, &found)
  /* count only */
  CHECK (APPROX (rec, n, pos_base, off, NULL, NULL, 0) == ACM_GPU_OK);
  CHECK (found == want_n);
  /* the exact room, with and without distances */
  ACMRecord *out = malloc ((want_n ? want_n : 1) * sizeof *out);
  uint32_t *dist = malloc ((want_n ? want_n : 1) * sizeof *dist);
  CHECK (out && dist);
  found = 0;
  CHECK (APPROX (rec, n, pos_base, off, out, dist, want_n) == ACM_GPU_OK);
  CHECK (found == want_n && same_records (out, want, want_n) && memcmp (dist, want_d, want_n * sizeof *dist) == 0);
  CHECK (APPROX (rec, n, pos_base, off, out, NULL, want_n) == ACM_GPU_OK && same_records (out, want, want_n));
  /* one short: nothing is written (the room of want_n - 1 entries is exact: a store would be seen) */
  if (want_n) {
    const size_t room = want_n - 1 ? want_n - 1 : 1;
    ACMRecord *tight = malloc (room * sizeof *tight);
    uint32_t *tight_d = malloc (room * sizeof *tight_d);
    CHECK (tight && tight_d);
    memset (tight, 0x5A, room * sizeof *tight);
    memset (tight_d, 0x5A, room * sizeof *tight_d);
    found = 0;
    CHECK (APPROX (rec, n, pos_base, off, tight, tight_d, want_n - 1) == ACM_GPU_E_OVERFLOW);
    CHECK (found == want_n);
    for (size_t b = 0; b < (want_n - 1) * sizeof *tight; b++)
      CHECK (((unsigned char *)tight)[b] == 0x5A);
    for (size_t b = 0; b < (want_n - 1) * sizeof *tight_d; b++)
      CHECK (((unsigned char *)tight_d)[b] == 0x5A);
    free (tight);
    free (tight_d);
  }
  /* refused: a record outside the buffer (its end, its start), of length 0; offsets that break the contract */
  if (n_rec) {
    memset (out, 0x5A, (want_n ? want_n : 1) * sizeof *out);
    const ACMRecord kept = rec[n_rec - 1];
    rec[n_rec - 1].end_pos = pos_base + n;
    CHECK (APPROX (rec, n, pos_base, off, out, dist, want_n) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    rec[n_rec - 1].length = (uint32_t)n + 1;
    CHECK (APPROX (rec, n, pos_base, off, out, dist, want_n) == ACM_GPU_E_ARG);
    rec[n_rec - 1].length = 0;
    CHECK (APPROX (rec, n, pos_base, off, out, dist, want_n) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    if (pos_base)
      CHECK (APPROX (rec, n, pos_base + n, off, out, dist, want_n) == ACM_GPU_E_ARG);
    if (off && n_texts >= 2 && off[1] < n) {
      const uint64_t cut = off[1];
      off[1] = n + 1;
      CHECK (APPROX (rec, n, pos_base, off, out, dist, want_n) == ACM_GPU_E_ARG);
      off[1] = cut;
      off[n_texts] = n - 1;
      CHECK (APPROX (rec, n, pos_base, off, out, dist, want_n) == ACM_GPU_E_ARG);
      off[n_texts] = n;
      off[0] = 1;
      CHECK (APPROX (rec, n, pos_base, off, out, dist, want_n) == ACM_GPU_E_ARG);
      off[0] = 0;
    }
    for (size_t b = 0; b < want_n * sizeof *out; b++)
      CHECK (((unsigned char *)out)[b] == 0x5A);
    CHECK (acm_approx_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, s.spell, s.spell_off, s.k, s.terms, s.tgt_ptr, N_TARGETS, nk, out, dist,
                               want_n, NULL) == ACM_GPU_E_ARG);
    CHECK (APPROX (rec, n, pos_base, off, NULL, dist, want_n ? want_n : 1) == ACM_GPU_E_ARG);
  }
#undef APPROX
  free (dist);
  free (out);
  free (want_d);
  free (want);
  free (rec);
  free (off);
  free (text);
  free_set (&s);
  return want_n;
}

int
main (void) {
  check_errors ();
  uint64_t matches = 0;
  /* exact and inexact occurrences, a target at the buffer's first and last symbol, seeds whose target would begin in front of
   * the buffer (`fgh` at 0) or end behind it (`abc` at the end) */
  static const char TEXT[] = "fgh abcdefgh abXdeYgh Xbcdefgh cdefg cdXfg cXeXg hab hXb Xab ab abcdefXh xbcdefgx hababc";
  matches += check_join (TEXT, NULL, 0, 0);
  matches += check_join (TEXT, NULL, 0, 1ull << 40);
  const uint64_t cuts[] = { 0, 0, 8, 21, 21, 32, 50, sizeof TEXT - 1, sizeof TEXT - 1 }; /* empty texts, a cut inside `abcdefgh`, a text that ends with a target */
  matches += check_join (TEXT, cuts, 8, 0);
  matches += check_join (TEXT, cuts, 8, 77);
  matches += check_join ("", NULL, 0, 0);
  matches += check_join ("zzzz", NULL, 0, 0);
  matches += check_join ("ab", NULL, 0, 3);
  CHECK (matches > 60);
  printf ("all checks held (%llu matches)\n", (unsigned long long)matches);
  return 0;
}
