/* Test-only driver: acm_near_check and acm_near_records (acm_host.c, no HIP) under AddressSanitizer and UBSan.
 * Every buffer is allocated at its exact size, so that a byte read or written beside it is seen.  The records
 * are made here by a naive loop over the text (every occurrence of every word, by end, longest first: the
 * canonical order), and the join is checked against a naive restatement of NEAR's definition written here: for
 * every group and end, every first symbol S downwards, the words of the group counted in the slice itself.  The
 * fixed case of tests/near_cases.py, 200 random cases and every contract error.  Built and run by
 * tests/test_near_sanitized.py; exits 0 when every check held. */
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

/* a set of groups over a list of words */
typedef struct {
  const char *const *words;
  int n_words;
  const uint32_t *terms;
  const uint64_t *group_ptr;
  const ACMNearGroup *groups;
  uint64_t n_groups;
} Set;

/* whether word w lies wholly inside text[S .. e], and whether it ends at e */
static int
word_inside (const char *text, size_t S, size_t e, const char *w, int *at_end) {
  const size_t len = strlen (w);
  int inside = 0;
  for (size_t s = S; s + len <= e + 1; s++)
    if (memcmp (text + s, w, len) == 0) {
      inside = 1;
      if (s + len == e + 1)
        *at_end = 1;
    }
  return inside;
}

/* NEAR from the text alone, in the total order: end ascending, length descending, group ascending */
static uint64_t
naive_near (const char *text, size_t n, const uint64_t *off, uint64_t n_texts, uint64_t pos_base, const Set *set, ACMRecord *out) {
  uint64_t k = 0;
  const uint64_t whole[2] = { 0, n };
  if (!off) {
    off = whole;
    n_texts = 1;
  }
  for (size_t e = 0; e < n; e++) {
    const uint64_t first = k;
    for (uint64_t g = 0; g < set->n_groups; g++)
      for (uint64_t t = 0; t < n_texts; t++) {
        if (!(off[t] <= e && e < off[t + 1]))
          continue;
        /* the shortest window that ends at e: every length from 1 up to the width and to the text's begin */
        const uint64_t m = set->group_ptr[g + 1] - set->group_ptr[g], need = set->groups[g].need ? set->groups[g].need : m;
        size_t shortest = 0;
        for (size_t l = 1; l <= set->groups[g].width && l <= e + 1 - off[t] && !shortest; l++) {
          uint64_t have = 0;
          int at_end = 0;
          for (uint64_t j = 0; j < m; j++)
            have += (uint64_t)word_inside (text, e + 1 - l, e, set->words[set->terms[set->group_ptr[g] + j]], &at_end);
          if (at_end && have >= need)
            shortest = l;
        }
        if (shortest)
          out[k++] = (ACMRecord){ pos_base + e, (uint32_t)shortest, (uint32_t)g };
      }
    for (uint64_t a = first + 1; a < k; a++) /* the matches of one end: the longest first, groups of one length stay in order */
      for (uint64_t b = a; b > first && out[b - 1].length < out[b].length; b--) {
        const ACMRecord t = out[b];
        out[b] = out[b - 1];
        out[b - 1] = t;
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

/* the fixed case of tests/near_cases.py */
static const char *const WORDS[] = { "he", "she", "his", "hers", "error", "disk", "timeout", "sda", "retry" };
enum { N_WORDS = 9 };
static const char TEXT[] = "error: disk sda timeout; retry\n"
                           "ushers: his disk error on sda, she hers\n"
                           "retry sda disk timeout error he\n"
                           "his error, her disk; timeout sda\n";
static const uint32_t TERMS[] = { 4, 5, 6, 8, 7, 0, 1, 3, 5, 7, 4, 5, 6, 7, 8, 6, 0, 2, 8 };
static const uint64_t GROUP_PTR[] = { 0, 2, 5, 8, 10, 15, 16, 19 };
static const ACMNearGroup GROUPS[] = { { 40, 0 }, { 30, 2 }, { 6, 2 }, { 20, 0 }, { 60, 3 }, { 5, 0 }, { 10, 1 } };
enum { N_GROUPS = 7, N_TERMS = 19 };

static void
check_errors (void) {
  uint32_t *terms = exact (TERMS, sizeof TERMS);
  uint64_t *ptr = exact (GROUP_PTR, sizeof GROUP_PTR);
  ACMNearGroup *groups = exact (GROUPS, sizeof GROUPS);
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_OK);
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS - 1) == ACM_GPU_E_ARG); /* keyword 8 */
  CHECK (acm_near_check (terms, NULL, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  CHECK (acm_near_check (NULL, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  CHECK (acm_near_check (terms, ptr, NULL, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  CHECK (acm_near_check (terms, ptr, groups, 1ull << 31, N_WORDS) == ACM_GPU_E_ARG); /* (refused before ptr is read that far) */
  uint64_t one = 0;
  CHECK (acm_near_check (NULL, &one, NULL, 0, 0) == ACM_GPU_OK); /* no group */
  ptr[3] = ptr[2];                                               /* a group without terms */
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[3] = 1; /* decreasing */
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[3] = GROUP_PTR[3];
  ptr[0] = 1;
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  ptr[0] = 0;
  terms[1] = 4; /* the same keyword twice in one group */
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  terms[1] = 5;
  groups[0].width = 0;
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  groups[0].width = ACM_NEAR_WIDTH_MAX;
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_OK);
  groups[0].width = ACM_NEAR_WIDTH_MAX + 1;
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  groups[0].width = 40;
  groups[0].need = 2; /* need = m */
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_OK);
  groups[0].need = 3;
  CHECK (acm_near_check (terms, ptr, groups, N_GROUPS, N_WORDS) == ACM_GPU_E_ARG);
  groups[0].need = 0;
  uint64_t far[2] = { 0, 1ull << 31 }; /* refused before terms[] is read */
  CHECK (acm_near_check (terms, far, groups, 1, N_WORDS) == ACM_GPU_E_ARG);
  far[1] = ACM_NEAR_TERMS_MAX + 1;
  CHECK (acm_near_check (terms, far, groups, 1, N_WORDS) == ACM_GPU_E_ARG);
  /* 16 distinct terms: the most */
  uint32_t many[ACM_NEAR_TERMS_MAX];
  for (uint32_t j = 0; j < ACM_NEAR_TERMS_MAX; j++)
    many[j] = j;
  far[1] = ACM_NEAR_TERMS_MAX;
  const ACMNearGroup all = { 9, ACM_NEAR_TERMS_MAX };
  CHECK (acm_near_check (many, far, &all, 1, ACM_NEAR_TERMS_MAX) == ACM_GPU_OK);
  free (groups);
  free (ptr);
  free (terms);
}

/* the join against the naive restatement over `text` cut at off[] (NULL: one text), at pos_base; then the overflow, the
 * count-only and the refused calls */
static uint64_t
check_join (const char *text, const uint64_t *off_in, uint64_t n_texts, uint64_t pos_base, const Set *set) {
  const size_t n = strlen (text);
  const uint64_t n_terms = set->group_ptr[set->n_groups], G = set->n_groups;
  uint32_t *terms = exact (set->terms, n_terms * sizeof *terms);
  uint64_t *ptr = exact (set->group_ptr, (G + 1) * sizeof *ptr);
  ACMNearGroup *groups = exact (set->groups, G * sizeof *groups);
  uint64_t *off = off_in ? exact (off_in, (n_texts + 1) * sizeof *off) : NULL;
  const uint64_t nk = (uint64_t)set->n_words;
  uint64_t n_rec = 0, found = 0;
  ACMRecord *rec = naive_records (text, n, set->words, set->n_words, pos_base, &n_rec);
  ACMRecord *most = malloc ((n * G + 1) * sizeof *most);
  CHECK (most);
  const uint64_t want_n = naive_near (text, n, off, n_texts, pos_base, set, most);
  ACMRecord *want = exact (most, want_n * sizeof *most);
  free (most);
  /* count only */
  CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, NULL, 0, &found) == ACM_GPU_OK);
  CHECK (found == want_n);
  /* the exact room */
  ACMRecord *out = malloc ((want_n ? want_n : 1) * sizeof *out);
  CHECK (out);
  found = 0;
  CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_OK);
  CHECK (found == want_n && same_records (out, want, want_n));
  /* one short: nothing is written (the room of want_n - 1 records is exact: a store would be seen) */
  if (want_n) {
    ACMRecord *tight = malloc ((want_n - 1 ? want_n - 1 : 1) * sizeof *tight);
    CHECK (tight);
    memset (tight, 0x5A, (want_n - 1 ? want_n - 1 : 1) * sizeof *tight);
    found = 0;
    CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, tight, want_n - 1, &found) == ACM_GPU_E_OVERFLOW);
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
    CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    rec[n_rec - 1].length = (uint32_t)n + 1;
    CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1].length = 0;
    CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
    rec[n_rec - 1] = kept;
    if (pos_base)
      CHECK (acm_near_records (rec, n_rec, n, pos_base + n, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
    if (off && n_texts >= 2 && off[1] < n) {
      const uint64_t cut = off[1];
      off[1] = n + 1;
      CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
      off[1] = cut;
      off[n_texts] = n - 1;
      CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
      off[n_texts] = n;
      off[0] = 1;
      CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
      off[0] = 0;
    }
    /* a set the check refuses, and missing arguments */
    groups[0].width = 0;
    CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
    groups[0].width = set->groups[0].width;
    CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, NULL) == ACM_GPU_E_ARG);
    CHECK (acm_near_records (rec, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, NULL, want_n ? want_n : 1, &found) == ACM_GPU_E_ARG);
    CHECK (acm_near_records (NULL, n_rec, n, pos_base, off, n_texts, terms, ptr, groups, G, nk, out, want_n, &found) == ACM_GPU_E_ARG);
    for (size_t b = 0; b < want_n * sizeof *out; b++)
      CHECK (((unsigned char *)out)[b] == 0x5A);
  }
  free (out);
  free (want);
  free (rec);
  free (off);
  free (groups);
  free (ptr);
  free (terms);
  return want_n;
}

/* a generator of the driver's own (a 64-bit LCG, the high bits) */
static uint64_t rng_state = 1975;
static uint32_t
rnd (uint32_t below) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((rng_state >> 33) % below);
}

/* 1 to 5 distinct words of 1 to 3 symbols over {a, b}, 1 to 4 groups of 1 to all of them with width 1 to 12 and need 0 to
 * m, a text of 0 to 40 symbols cut into 1 to 4 texts (empty ones included) */
static uint64_t
check_random (void) {
  char spell[5][4];
  const char *words[5];
  int n_words = 0;
  for (uint32_t tries = 1 + rnd (5); tries; tries--) {
    char w[4] = { 0 };
    const uint32_t len = 1 + rnd (3);
    for (uint32_t i = 0; i < len; i++)
      w[i] = (char)('a' + rnd (2));
    int known = 0;
    for (int k = 0; k < n_words; k++)
      known = known || strcmp (spell[k], w) == 0;
    if (!known) {
      memcpy (spell[n_words], w, 4);
      words[n_words] = spell[n_words];
      n_words++;
    }
  }
  uint32_t terms[4 * 5];
  uint64_t ptr[5] = { 0 };
  ACMNearGroup groups[4];
  const uint32_t n_groups = 1 + rnd (4);
  for (uint32_t g = 0; g < n_groups; g++) {
    uint32_t ids[5] = { 0, 1, 2, 3, 4 };
    for (uint32_t i = (uint32_t)n_words - 1; i > 0; i--) { /* a shuffle: the group takes its first m */
      const uint32_t j = rnd (i + 1), t = ids[i];
      ids[i] = ids[j];
      ids[j] = t;
    }
    const uint32_t m = 1 + rnd ((uint32_t)n_words);
    memcpy (terms + ptr[g], ids, m * sizeof *ids);
    ptr[g + 1] = ptr[g] + m;
    groups[g] = (ACMNearGroup){ 1 + rnd (12), rnd (m + 1) };
  }
  char text[41] = { 0 };
  const uint32_t n = rnd (41);
  for (uint32_t i = 0; i < n; i++)
    text[i] = (char)('a' + rnd (2));
  uint64_t off[5] = { 0 };
  const uint32_t n_cuts = rnd (4);
  for (uint32_t c = 1; c <= n_cuts; c++) {
    off[c] = rnd (n + 1);
    for (uint32_t d = c; d > 1 && off[d] < off[d - 1]; d--) { /* (kept in order) */
      const uint64_t t = off[d];
      off[d] = off[d - 1];
      off[d - 1] = t;
    }
  }
  off[n_cuts + 1] = n;
  const Set set = { words, n_words, terms, ptr, groups, n_groups };
  return check_join (text, off, n_cuts + 1, rnd (2) ? 0 : (1ull << 32) - 20, &set);
}

/* 600 x `a` under the words a, aa, aaa and a group that also needs a `b` that never comes: no match, and every record is
 * looked at; then the same group with need 2 */
static void
check_dense (void) {
  enum { A = 600 };
  char text[A + 1];
  memset (text, 'a', A);
  text[A] = 0;
  static const char *const words[] = { "a", "aa", "aaa", "b" };
  const uint32_t terms[] = { 0, 1, 3 };
  const uint64_t ptr[] = { 0, 3 };
  ACMNearGroup group = { ACM_NEAR_WIDTH_MAX, 0 };
  uint64_t n_rec = 0, found = 77;
  ACMRecord *rec = naive_records (text, A, words, 4, 0, &n_rec);
  CHECK (n_rec == 3 * A - 3);
  ACMRecord *out = malloc (A * sizeof *out);
  CHECK (out);
  CHECK (acm_near_records (rec, n_rec, A, 0, NULL, 0, terms, ptr, &group, 1, 4, out, A, &found) == ACM_GPU_OK && found == 0);
  group.need = 2;
  CHECK (acm_near_records (rec, n_rec, A, 0, NULL, 0, terms, ptr, &group, 1, 4, out, A, &found) == ACM_GPU_OK && found == A - 1);
  for (uint64_t j = 0; j < found; j++) /* `aa` ends at e and holds an `a` */
    CHECK (out[j].end_pos == j + 1 && out[j].length == 2 && out[j].keyword_id == 0);
  /* no record at all, and no symbol at all */
  CHECK (acm_near_records (NULL, 0, A, 0, NULL, 0, terms, ptr, &group, 1, 4, out, A, &found) == ACM_GPU_OK && found == 0);
  const uint64_t none[1] = { 0 };
  CHECK (acm_near_records (NULL, 0, 0, 0, none, 0, terms, ptr, &group, 1, 4, NULL, 0, &found) == ACM_GPU_OK && found == 0);
  free (out);
  free (rec);
}

int
main (void) {
  check_errors ();
  const Set fixed = { WORDS, N_WORDS, TERMS, GROUP_PTR, GROUPS, N_GROUPS };
  const uint64_t n = sizeof TEXT - 1;
  uint64_t matches = 0;
  const uint64_t whole = check_join (TEXT, NULL, 0, 0, &fixed);
  CHECK (whole >= 20);
  matches += whole;
  matches += check_join (TEXT, NULL, 0, (1ull << 32) - 20, &fixed);
  matches += check_join (TEXT, NULL, 0, (1ull << 63) + 5, &fixed);
  const uint64_t cut[] = { 0, 88, n };
  const uint64_t lost = whole - check_join (TEXT, cut, 2, 0, &fixed);
  CHECK (lost >= 1 && lost < whole);
  const uint64_t cuts[] = { 0, 0, 31, 31, 45, 71, 103, n, n }; /* empty texts, the lines, a cut inside the second line */
  matches += check_join (TEXT, cuts, 8, 77, &fixed);
  matches += check_join ("", NULL, 0, 0, &fixed);
  matches += check_join ("zzzz", NULL, 0, 0, &fixed);
  uint64_t random_matches = 0, nonempty = 0;
  for (int trial = 0; trial < 200; trial++) {
    const uint64_t got = check_random ();
    random_matches += got;
    nonempty += got != 0;
  }
  CHECK (nonempty >= 100);
  check_dense ();
  printf ("all checks held (%llu matches, %llu in %llu of 200 random cases)\n", (unsigned long long)matches, (unsigned long long)random_matches,
          (unsigned long long)nonempty);
  return 0;
}
