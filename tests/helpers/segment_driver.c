/* Test-only driver: acm_segment_records and the caller-loop acm_segment (acm_host.c, no HIP) under
 * AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte read or
 * written beside it is seen.  The answer is checked against the definition of SEGMENT written here
 * position by position (include/acm_segment.h), and its cost against the minimum over all tilings of
 * the small sets.  What acm_segment would run for a machine no GPU path takes is
 * acm_internal_cpu_segment, and that function is called here as acm_segment calls it (acm_segment
 * itself lives in the HIP translation unit, which this program does not link).
 * Built and run by tests/test_segment_sanitized.py; exits 0 when every check held. */
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

/* every occurrence of every keyword in canonical order: end ascending, longest first */
static uint64_t
naive (const char *text, size_t n, const char *const *words, int n_words, ACMRecord *out) {
  uint64_t k = 0;
  for (size_t e = 0; e < n; e++)
    for (size_t len = e + 1; len >= 1; len--)
      for (int w = 0; w < n_words; w++)
        if (strlen (words[w]) == len && memcmp (text + e + 1 - len, words[w], len) == 0) {
          if (out) {
            out[k].end_pos = e;
            out[k].length = (uint32_t)len;
            out[k].keyword_id = (uint32_t)w;
          }
          k++;
        }
  return k;
}

/* the definition over positions 0 .. n: the emitted records into out (ascending), their number returned, best[n] in *total */
static uint64_t
define (const ACMRecord *rec, uint64_t m, const uint32_t *cost, uint32_t gap, size_t n, ACMRecord *out, uint64_t *total) {
  uint64_t *best = malloc ((n + 1) * sizeof *best);
  ACMRecord *rev = malloc ((m ? m : 1) * sizeof *rev);
  CHECK (best && rev);
  best[0] = 0;
  for (size_t p = 1; p <= n; p++) {
    best[p] = best[p - 1] + gap;
    for (uint64_t i = 0; i < m; i++)
      if (rec[i].end_pos == p - 1 && best[p - rec[i].length] + cost[rec[i].keyword_id] < best[p])
        best[p] = best[p - rec[i].length] + cost[rec[i].keyword_id];
  }
  uint64_t k = 0;
  for (size_t p = n; p > 0;) {
    uint64_t take = m;
    for (uint64_t i = 0; i < m; i++)
      if (rec[i].end_pos == p - 1 && best[p - rec[i].length] + cost[rec[i].keyword_id] == best[p] &&
          (take == m || rec[i].length > rec[take].length || (rec[i].length == rec[take].length && rec[i].keyword_id < rec[take].keyword_id)))
        take = i;
    if (take != m) {
      rev[k++] = rec[take];
      p -= rec[take].length;
    } else
      p--;
  }
  for (uint64_t j = 0; j < k; j++)
    out[j] = rev[k - 1 - j];
  *total = best[n];
  free (rev), free (best);
  return k;
}

/* the least cost over all tilings of at most 16 records */
static uint64_t
exhaustive (const ACMRecord *rec, uint64_t m, const uint32_t *cost, uint32_t gap, size_t n) {
  uint64_t least = (uint64_t)gap * n;
  for (uint32_t mask = 1; mask < (1u << m); mask++) {
    uint64_t c = 0, covered = 0;
    int ok = 1;
    for (uint64_t i = 0; i < m && ok; i++)
      if (mask >> i & 1) {
        for (uint64_t j = 0; j < i; j++)
          if ((mask >> j & 1) && rec[j].end_pos >= rec[i].end_pos + 1 - rec[i].length && rec[i].end_pos >= rec[j].end_pos + 1 - rec[j].length)
            ok = 0;
        c += cost[rec[i].keyword_id];
        covered += rec[i].length;
      }
    if (ok && c + gap * (n - covered) < least)
      least = c + gap * (n - covered);
  }
  return least;
}

static uint32_t rng_state = 1975;
static uint32_t
rnd (uint32_t below) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % below;
}

/* one case through acm_segment_records, buffers at their exact sizes */
static void
run_case (const char *text, size_t n, const char *const *words, int n_words, const uint32_t *cost_in, uint32_t gap, uint64_t shift) {
  const uint64_t m = naive (text, n, words, n_words, NULL);
  ACMRecord *rec = malloc ((m ? m : 1) * sizeof *rec), *want = malloc ((m ? m : 1) * sizeof *want), *buf = malloc ((m ? m : 1) * sizeof *buf);
  uint32_t *cost = malloc ((size_t)n_words * sizeof *cost);
  CHECK (rec && want && buf && cost);
  memcpy (cost, cost_in, (size_t)n_words * sizeof *cost);
  (void)naive (text, n, words, n_words, rec);
  uint64_t total = 0;
  const uint64_t n_want = define (rec, m, cost, gap, n, want, &total);
  if (m <= 16)
    CHECK (exhaustive (rec, m, cost, gap, n) == total);
  memcpy (buf, rec, m * sizeof *rec);
  for (uint64_t j = 0; j < m; j++)
    buf[j].end_pos += shift;
  uint64_t got = 99, sums[2] = { 99, 99 };
  CHECK (acm_segment_records (m ? buf : NULL, m, cost, (uint64_t)n_words, gap, &got, sums) == ACM_GPU_OK);
  CHECK (got == n_want);
  uint64_t sum_len = 0;
  for (uint64_t j = 0; j < got; j++) {
    CHECK (buf[j].end_pos == want[j].end_pos + shift && buf[j].length == want[j].length && buf[j].keyword_id == want[j].keyword_id);
    sum_len += buf[j].length;
  }
  CHECK (sums[1] == sum_len && sums[0] + gap * (n - sums[1]) == total);
  free (cost), free (buf), free (want), free (rec);
}

static int
cmp8 (const void *a, const void *b, const void *arg) {
  (void)arg;
  return memcmp (a, b, 8);
}

int
main (void) {
  /* the worked examples of the header */
  {
    const char *w1[4] = { "he", "she", "his", "hers" }, *w2[3] = { "ab", "abc", "cd" }, *w3[2] = { "a", "aa" }, *w4[3] = { "a", "aa", "aaa" };
    const uint32_t c1[4] = { 1, 1, 1, 1 }, c2[3] = { 1, 1, 1 }, c3[2] = { 2, 4 }, c4[3] = { 5, 6, 100 };
    char *as = malloc (1001);
    CHECK (as);
    memset (as, 'a', 1001);
    run_case ("ushers", 6, w1, 4, c1, 2, 0);
    run_case ("abcd", 4, w2, 3, c2, 10, 0);
    run_case (as, 1001, w3, 2, c3, 2, 0);
    run_case (as, 1000, w4, 3, c4, 7, 1ull << 33);
    free (as);
  }
  /* random cases over two or three letters, costs and gap in 0 .. 7, zero included */
  for (int round = 0; round < 300; round++) {
    char words[8][8], text[64];
    const char *ptr[8];
    const uint32_t alpha = 2 + rnd (2);
    const int n_words = 2 + (int)rnd (7);
    uint32_t cost[8];
    for (int w = 0; w < n_words; w++) {
      const uint32_t len = 1 + rnd (6);
      for (uint32_t i = 0; i < len; i++)
        words[w][i] = (char)('a' + rnd (alpha));
      words[w][len] = 0;
      for (int v = 0; v < w; v++) /* distinct keywords: a duplicate gets a letter the text lacks */
        if (strcmp (words[v], words[w]) == 0)
          words[w][0] = (char)('q' + w);
      ptr[w] = words[w];
      cost[w] = rnd (8);
    }
    const size_t n = 1 + rnd (round < 150 ? 8 : 60);
    for (size_t i = 0; i < n; i++)
      text[i] = (char)('a' + rnd (alpha));
    run_case (text, n, ptr, n_words, cost, rnd (8), round % 3 ? 0 : 1ull << 33);
  }
  /* refused, nothing modified; none and one record */
  {
    const char *w[4] = { "he", "she", "his", "hers" };
    uint32_t *cost = malloc (4 * sizeof *cost);
    ACMRecord *rec = malloc (3 * sizeof *rec), *copy = malloc (3 * sizeof *copy);
    CHECK (cost && rec && copy);
    CHECK (naive ("ushers", 6, w, 4, rec) == 3);
    memcpy (copy, rec, 3 * sizeof *rec);
    uint64_t got = 99;
    cost[0] = cost[1] = cost[2] = 1, cost[3] = 1u << 24;
    CHECK (acm_segment_records (rec, 3, cost, 4, 2, &got, NULL) == ACM_GPU_E_ARG);
    cost[3] = 1;
    CHECK (acm_segment_records (rec, 3, cost, 4, 1u << 24, &got, NULL) == ACM_GPU_E_ARG);
    CHECK (acm_segment_records (rec, 3, cost, 3, 2, &got, NULL) == ACM_GPU_E_ARG); /* `hers` is keyword 3 */
    CHECK (acm_segment_records (rec, 3, NULL, 4, 2, &got, NULL) == ACM_GPU_E_ARG);
    CHECK (acm_segment_records (NULL, 3, cost, 4, 2, &got, NULL) == ACM_GPU_E_ARG);
    CHECK (acm_segment_records (rec, 3, cost, 4, 2, NULL, NULL) == ACM_GPU_E_ARG);
    rec[1].length = 0;
    CHECK (acm_segment_records (rec, 3, cost, 4, 2, &got, NULL) == ACM_GPU_E_ARG);
    rec[1].length = copy[1].length;
    rec[2].end_pos = 1;
    CHECK (acm_segment_records (rec, 3, cost, 4, 2, &got, NULL) == ACM_GPU_E_ARG); /* ends that descend */
    rec[2].end_pos = (1ull << 41);
    CHECK (acm_segment_records (rec, 3, cost, 4, 2, &got, NULL) == ACM_GPU_E_ARG); /* a span of 2^40 or more */
    rec[2].end_pos = copy[2].end_pos;
    CHECK (got == 99 && memcmp (rec, copy, 3 * sizeof *rec) == 0);
    uint64_t sums[2] = { 9, 9 };
    CHECK (acm_segment_records (NULL, 0, NULL, 0, 0, &got, sums) == ACM_GPU_OK && got == 0 && sums[0] == 0 && sums[1] == 0);
    CHECK (acm_segment_records (rec, 3, cost, 4, (1u << 24) - 1, &got, sums) == ACM_GPU_OK && got == 1 && rec[0].keyword_id == 3); /* the largest gap cost: `hers` covers the most symbols */
    free (copy), free (rec), free (cost);
  }

  /* the caller loop of a machine over 8-byte symbols, then SEGMENT: acm_segment's host path */
  {
    const char *w[4] = { "he", "she", "his", "hers" };
    const char *flat = "ushers, his hers; she";
    const size_t n = strlen (flat);
    ACMachine *m = acm_create (cmp8, 0, 0);
    unsigned char *letters[4];
    for (int k = 0; k < 4; k++) {
      const size_t len = strlen (w[k]);
      letters[k] = calloc (len, 8);
      CHECK (letters[k]);
      const ACState *s = acm_initiate (m);
      for (size_t i = 0; i < len; i++) {
        letters[k][8 * i] = (unsigned char)w[k][i];
        acm_insert_letter_of_keyword (&s, letters[k] + 8 * i);
      }
      acm_insert_end_of_keyword (&s, 0, 0);
    }
    CHECK (acm_set_symbol_bytes (m, 8) == ACM_GPU_OK);
    unsigned char *text = calloc (n, 8);
    CHECK (text);
    for (size_t i = 0; i < n; i++)
      text[8 * i] = (unsigned char)flat[i];
    const uint64_t n_all = naive (flat, n, w, 4, NULL);
    ACMRecord *all = malloc (n_all * sizeof *all), *want = malloc (n_all * sizeof *want), *rec = malloc (n_all * sizeof *rec); /* room for ALL matches, exactly */
    uint32_t *cost = malloc (4 * sizeof *cost);
    CHECK (all && want && rec && cost);
    cost[0] = 1, cost[1] = 2, cost[2] = 3, cost[3] = 1;
    (void)naive (flat, n, w, 4, all);
    uint64_t total = 0, found = 99, sums[2] = { 0, 0 };
    const uint64_t n_want = define (all, n_all, cost, 2, n, want, &total);
    CHECK (n_want > 0 && n_want < n_all);
    CHECK (acm_internal_cpu_segment (m, text, n, 8, cost, 4, 2, rec, n_all, &found, sums) == ACM_GPU_OK);
    CHECK (found == n_want && memcmp (rec, want, found * sizeof *rec) == 0 && sums[0] + 2 * (n - sums[1]) == total);
    CHECK (acm_internal_cpu_segment (m, text, n, 8, cost, 4, 2, rec, n_all - 1, &found, sums) == ACM_GPU_E_OVERFLOW && found == n_all);
    CHECK (acm_internal_cpu_segment (m, text, n, 8, cost, 3, 2, rec, n_all, &found, sums) == ACM_GPU_E_ARG); /* the table misses a keyword */
    cost[3] = 1u << 24;
    CHECK (acm_internal_cpu_segment (m, text, n, 8, cost, 4, 2, rec, n_all, &found, sums) == ACM_GPU_E_ARG);
    cost[3] = 1;
    found = 99;
    CHECK (acm_internal_cpu_segment (m, NULL, 0, 8, cost, 4, 2, NULL, 0, &found, sums) == ACM_GPU_OK && found == 0);
    free (cost), free (rec), free (want), free (all), free (text);
    acm_release (m);
    for (int k = 0; k < 4; k++)
      free (letters[k]);
  }
  printf ("all checks held\n");
  return 0;
}
