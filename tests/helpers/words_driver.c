/* Test-only driver: acm_words_records and the caller-loop acm_scan_words (acm_host.c, no HIP) under
 * AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte read or
 * written beside it is seen: a record at symbol 0 and one that ends at n - 1 have no neighbour inside
 * the buffer.  The filter is checked against a naive loop written here.  The machine's comparator is
 * memcmp over 8-byte symbols, declared with acm_set_symbol_bytes: what acm_scan_words would run for it
 * is acm_internal_cpu_scan_words, and that function is called here as acm_scan_words calls it
 * (acm_scan_words itself lives in the HIP translation unit, which this program does not link).
 * Built and run by tests/test_words_sanitized.py; exits 0 when every check held. */
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

/* the letter c as a little-endian symbol of sb bytes: c in the lowest byte, 0x41 in the highest of a wider one */
static unsigned char *
widen (const char *word, size_t n, size_t sb) {
  unsigned char *to = malloc (n * sb ? n * sb : 1);
  CHECK (to);
  memset (to, 0, n * sb ? n * sb : 1);
  for (size_t i = 0; i < n; i++) {
    to[sb * i] = (unsigned char)word[i];
    if (sb > 1)
      to[sb * i + sb - 1] = 0x41;
  }
  return to;
}

static int
word_char (char c) {
  return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || c == '_' || (c >= 'a' && c <= 'z');
}

/* the definition, letter by letter, over every occurrence of every keyword in order of (end, longest first): the
 * records kept under `flags`, as (end_pos, length, keyword) triples */
static uint64_t
naive (const char *text, size_t n, const uint64_t *off, uint64_t n_texts, const char *const *words, int n_words, uint32_t flags, int all,
       ACMRecord *out) {
  uint64_t k = 0;
  for (size_t e = 0; e < n; e++)
    for (size_t len = n; len >= 1; len--)
      for (int w = 0; w < n_words; w++) {
        if (strlen (words[w]) != len || len > e + 1 || memcmp (text + e + 1 - len, words[w], len) != 0)
          continue;
        const size_t s = e + 1 - len;
        uint64_t t = 0;
        for (uint64_t j = 0; j < n_texts; j++)
          if (off[j] <= s)
            t = j;
        int keep = 1;
        if (!all) {
          if (e >= off[t + 1])
            keep = 0;
          else {
            const int left_ok = s == off[t] || !word_char (text[s - 1]), right_ok = e + 1 == off[t + 1] || !word_char (text[e + 1]);
            keep = (!(flags & ACM_WORDS_LEFT) || left_ok) && (!(flags & ACM_WORDS_RIGHT) || right_ok);
          }
        }
        if (keep) {
          out[k].end_pos = e;
          out[k].length = (uint32_t)len;
          out[k].keyword_id = (uint32_t)w;
          k++;
        }
      }
  return k;
}

static int
cmp8 (const void *a, const void *b, const void *arg) {
  (void)arg;
  return memcmp (a, b, 8);
}

int
main (void) {
  const char *words[5] = { "he", "she", "hers", "x", "e.g." };
  /* records at symbol 0 and at n - 1 in every text; empty texts; a match that spans a cut */
  const char *flat = "he shehers_x e.g.ushers x";
  const size_t n = strlen (flat);
  const uint64_t one[2] = { 0, n };
  const uint64_t cuts[9] = { 0, 0, 2, 6, 6, 6, 12, 19, n }; /* "", "he", " she", "", "", "hers_x", " e.g.us", "hers x" */
  const size_t sizes[] = { 1, 2, 4, 8 };
  const char *ascii = "09AZ__az";
  ACMRecord *all = malloc (4 * n * sizeof *all), *want = malloc (4 * n * sizeof *want);
  CHECK (all && want);
  const uint64_t n_all = naive (flat, n, one, 1, words, 5, 0, 1, all);
  CHECK (n_all > 8);
  for (size_t c = 0; c < sizeof sizes / sizeof *sizes; c++)
    for (int batch = 0; batch < 2; batch++)
      for (uint32_t flags = ACM_WORDS_LEFT; flags <= ACM_WORDS_BOTH; flags++) {
        const size_t sb = sizes[c];
        unsigned char *text = widen (flat, n, sb), *ranges = widen (ascii, 8, sb);
        const uint64_t n_want = naive (flat, n, batch ? cuts : one, batch ? 8 : 1, words, 5, flags, 0, want);
        CHECK (n_want > 0 && n_want < n_all);
        ACMRecord *rec = malloc (n_all * sizeof *rec); /* exactly the records */
        CHECK (rec);
        memcpy (rec, all, n_all * sizeof *rec);
        for (uint64_t j = 0; j < n_all; j++)
          rec[j].end_pos += 77;
        uint64_t kept = 99;
        CHECK (acm_words_records (text, n, (uint32_t)sb, 77, batch ? cuts : NULL, batch ? 8 : 0, ranges, 4, flags, rec, n_all, &kept) == ACM_GPU_OK);
        CHECK (kept == n_want);
        for (uint64_t j = 0; j < kept; j++)
          CHECK (rec[j].end_pos == want[j].end_pos + 77 && rec[j].length == want[j].length && rec[j].keyword_id == want[j].keyword_id);
        free (rec), free (ranges), free (text);
      }
  /* 16 ranges of 8-byte symbols: the ASCII set cut into 16, s-t last */
  {
    const char *sixteen = "09AZ__abcdefghijklmnopqruvwxyzst";
    unsigned char *text = widen (flat, n, 8), *ranges = widen (sixteen, 32, 8);
    const uint64_t n_want = naive (flat, n, one, 1, words, 5, ACM_WORDS_BOTH, 0, want);
    ACMRecord *rec = malloc (n_all * sizeof *rec);
    CHECK (rec);
    memcpy (rec, all, n_all * sizeof *rec);
    uint64_t kept = 99;
    CHECK (acm_words_records (text, n, 8, 0, NULL, 0, ranges, 16, ACM_WORDS_BOTH, rec, n_all, &kept) == ACM_GPU_OK);
    CHECK (kept == n_want && memcmp (rec, want, kept * sizeof *rec) == 0);
    memcpy (rec, all, n_all * sizeof *rec);
    CHECK (acm_words_records (text, n, 8, 0, NULL, 0, ranges, 15, ACM_WORDS_BOTH, rec, n_all, &kept) == ACM_GPU_OK);
    CHECK (kept > n_want); /* without s-t, "hers" of "ushers x" is a whole word */
    /* refused, nothing modified */
    memcpy (rec, all, n_all * sizeof *rec);
    CHECK (acm_words_records (text, n, 8, 0, NULL, 0, ranges, 17, ACM_WORDS_BOTH, rec, n_all, &kept) == ACM_GPU_E_ARG);
    CHECK (acm_words_records (text, n, 8, 0, NULL, 0, ranges, 16, 0, rec, n_all, &kept) == ACM_GPU_E_ARG);
    CHECK (acm_words_records (text, n, 8, 0, NULL, 0, ranges, 16, 4, rec, n_all, &kept) == ACM_GPU_E_ARG);
    CHECK (acm_words_records (text, n, 3, 0, NULL, 0, ranges, 16, ACM_WORDS_BOTH, rec, n_all, &kept) == ACM_GPU_E_ARG);
    CHECK (acm_words_records (text, n - 1, 8, 0, NULL, 0, ranges, 16, ACM_WORDS_BOTH, rec, n_all, &kept) == ACM_GPU_E_ARG); /* the last record ends at n - 1 */
    CHECK (acm_words_records (text, n, 8, 1, NULL, 0, ranges, 16, ACM_WORDS_BOTH, rec, n_all, &kept) == ACM_GPU_E_ARG);     /* the first begins at 0 */
    const uint64_t bad_cuts[3] = { 0, 9, 7 };
    CHECK (acm_words_records (text, n, 8, 0, bad_cuts, 2, ranges, 16, ACM_WORDS_BOTH, rec, n_all, &kept) == ACM_GPU_E_ARG);
    CHECK (memcmp (rec, all, n_all * sizeof *rec) == 0);
    /* no record, no text */
    kept = 99;
    CHECK (acm_words_records (NULL, 0, 8, 0, NULL, 0, ranges, 16, ACM_WORDS_BOTH, NULL, 0, &kept) == ACM_GPU_OK && kept == 0);
    free (rec), free (ranges), free (text);
  }

  /* the caller loop of a machine over 8-byte symbols, then the filter: acm_scan_words' host path */
  ACMachine *m = acm_create (cmp8, 0, 0);
  unsigned char *letters[5];
  for (int k = 0; k < 5; k++) {
    const size_t len = strlen (words[k]);
    letters[k] = widen (words[k], len, 8);
    const ACState *s = acm_initiate (m);
    for (size_t i = 0; i < len; i++)
      acm_insert_letter_of_keyword (&s, letters[k] + 8 * i);
    acm_insert_end_of_keyword (&s, 0, 0);
  }
  CHECK (acm_set_symbol_bytes (m, 8) == ACM_GPU_OK);
  unsigned char *text = widen (flat, n, 8), *ranges = widen (ascii, 8, 8);
  for (uint32_t flags = ACM_WORDS_LEFT; flags <= ACM_WORDS_BOTH; flags++) {
    const uint64_t n_want = naive (flat, n, one, 1, words, 5, flags, 0, want);
    ACMRecord *rec = malloc (n_all * sizeof *rec); /* room for ALL matches, exactly */
    CHECK (rec);
    uint64_t found = 99;
    CHECK (acm_internal_cpu_scan_words (m, text, n, 8, ranges, 4, flags, rec, n_all, &found) == ACM_GPU_OK);
    CHECK (found == n_want && memcmp (rec, want, found * sizeof *rec) == 0);
    free (rec);
  }
  {
    ACMRecord *rec = malloc ((n_all - 1) * sizeof *rec); /* one too little: the count that suffices */
    CHECK (rec);
    uint64_t found = 99;
    CHECK (acm_internal_cpu_scan_words (m, text, n, 8, ranges, 4, ACM_WORDS_BOTH, rec, n_all - 1, &found) == ACM_GPU_E_OVERFLOW && found == n_all);
    CHECK (acm_internal_cpu_scan_words (m, text, n, 8, ranges, 4, 0, rec, n_all - 1, &found) == ACM_GPU_E_ARG);
    CHECK (acm_internal_cpu_scan_words (m, text, n, 3, ranges, 4, ACM_WORDS_BOTH, rec, n_all - 1, &found) == ACM_GPU_E_ARG);
    found = 99;
    CHECK (acm_internal_cpu_scan_words (m, NULL, 0, 8, ranges, 4, ACM_WORDS_BOTH, NULL, 0, &found) == ACM_GPU_OK && found == 0);
    free (rec);
  }
  free (ranges), free (text);
  acm_release (m);
  for (int k = 0; k < 5; k++)
    free (letters[k]);
  free (want), free (all);
  printf ("all checks held\n");
  return 0;
}
