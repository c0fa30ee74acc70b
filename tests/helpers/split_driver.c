/* Test-only driver: acm_split_offsets and the caller-loop acm_grep_lines (acm_host.c, no HIP) under
 * AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte read or
 * written beside it is seen.  The split is checked against a naive loop written here.  The machine's
 * comparator is memcmp over 3-byte symbols, declared with acm_set_symbol_bytes: what acm_grep_lines
 * would run for it is acm_internal_cpu_grep_lines, and that function is called here as acm_grep_lines
 * calls it (acm_grep_lines itself lives in the HIP translation unit, which this program does not
 * link).  Built and run by tests/test_split_sanitized.py; exits 0 when every check held. */
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

/* the letter c as a symbol of sb bytes: (c, c ^ 0x5A, 7, 8, ...) */
static unsigned char *
widen (const char *word, size_t n, size_t sb) {
  unsigned char *to = malloc (n * sb ? n * sb : 1);
  CHECK (to);
  for (size_t i = 0; i < n; i++)
    for (size_t b = 0; b < sb; b++)
      to[sb * i + b] = b == 0 ? (unsigned char)word[i] : b == 1 ? (unsigned char)word[i] ^ 0x5A : (unsigned char)(5 + b);
  return to;
}

static int
is_delim (char c, const char *delims) {
  return c && strchr (delims, c) != NULL;
}

/* the definition, letter by letter: offsets into want[], the number of cuts returned */
static uint64_t
naive (const char *text, size_t n, const char *delims, int runs, uint64_t *want) {
  uint64_t k = 0;
  want[0] = 0;
  for (size_t i = 0; i < n; i++) {
    int cut = is_delim (text[i], delims);
    if (runs && cut && i + 1 < n && is_delim (text[i + 1], delims))
      cut = 0;
    if (i + 1 == n)
      cut = 1;
    if (cut)
      want[++k] = i + 1;
  }
  return k;
}

static int
cmp3 (const void *a, const void *b, const void *arg) {
  (void)arg;
  return memcmp (a, b, 3);
}

int
main (void) {
  const char *texts[] = { "", "\n", "a", "abcxyz", "\n\n\n\n", "ab\ncd\n", "ab\ncd", "\n\n\nab\n\ncd", "a\n\nb", "ab \t\ncd, ef\n\n", " \t lead" };
  const char *delim_sets[] = { "\n", " \t\n,", "\n\t ,;.:!?()[]{}-" };
  const size_t sizes[] = { 1, 2, 3, 4, 8 };
  for (size_t a = 0; a < sizeof texts / sizeof *texts; a++)
    for (size_t b = 0; b < sizeof delim_sets / sizeof *delim_sets; b++)
      for (size_t c = 0; c < sizeof sizes / sizeof *sizes; c++)
        for (int runs = 0; runs < 2; runs++) {
          const size_t n = strlen (texts[a]), nd = strlen (delim_sets[b]), sb = sizes[c];
          unsigned char *text = widen (texts[a], n, sb), *delims = widen (delim_sets[b], nd, sb);
          uint64_t *want = malloc ((n + 1) * sizeof *want);
          CHECK (want);
          const uint64_t k = naive (texts[a], n, delim_sets[b], runs, want);
          uint64_t got_n = 99;
          /* count only */
          CHECK (acm_split_offsets (n ? text : NULL, n, (uint32_t)sb, delims, (uint32_t)nd, (uint32_t)runs, NULL, 0, &got_n) == ACM_GPU_OK);
          CHECK (got_n == k);
          /* exactly the room */
          uint64_t *off = malloc ((k + 1) * sizeof *off);
          CHECK (off);
          got_n = 99;
          CHECK (acm_split_offsets (n ? text : NULL, n, (uint32_t)sb, delims, (uint32_t)nd, (uint32_t)runs, off, k, &got_n) == ACM_GPU_OK);
          CHECK (got_n == k && memcmp (off, want, (k + 1) * sizeof *off) == 0);
          free (off);
          /* one too little: the count, nothing written (the array has k entries: one write too many is seen) */
          if (k) {
            off = malloc (k * sizeof *off);
            CHECK (off);
            memset (off, 0xA5, k * sizeof *off);
            got_n = 99;
            CHECK (acm_split_offsets (text, n, (uint32_t)sb, delims, (uint32_t)nd, (uint32_t)runs, off, k - 1, &got_n) == ACM_GPU_E_OVERFLOW);
            CHECK (got_n == k);
            for (uint64_t i = 0; i < k; i++)
              CHECK (off[i] == 0xA5A5A5A5A5A5A5A5ull);
            free (off);
          }
          free (want), free (delims), free (text);
        }
  uint64_t n_bad = 0;
  CHECK (acm_split_offsets ("a", 1, 1, "\n", 0, 0, NULL, 0, &n_bad) == ACM_GPU_E_ARG);
  CHECK (acm_split_offsets ("a", 1, 1, "\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n", 17, 0, NULL, 0, &n_bad) == ACM_GPU_E_ARG);
  CHECK (acm_split_offsets ("a", 1, 1, "\n", 1, 2, NULL, 0, &n_bad) == ACM_GPU_E_ARG);

  /* {he, she, hers, s} over "\nus\nhers and sh\ne sells she\n\non top\n" cut at newlines and at "r": the texts
   * "\n", "us\n", "her", "s and sh\n", "e sells she\n", "\n", "on top\n" */
  ACMachine *m = acm_create (cmp3, 0, 0);
  const char *words[4] = { "he", "she", "hers", "s" };
  unsigned char *letters[4];
  for (int k = 0; k < 4; k++) {
    const size_t n = strlen (words[k]);
    letters[k] = widen (words[k], n, 3);
    const ACState *s = acm_initiate (m);
    for (size_t i = 0; i < n; i++)
      acm_insert_letter_of_keyword (&s, letters[k] + 3 * i);
    acm_insert_end_of_keyword (&s, 0, 0);
  }
  CHECK (acm_set_symbol_bytes (m, 3) == ACM_GPU_OK);
  const char *flat = "\nus\nhers and sh\ne sells she\n\non top\n";
  const uint64_t n_sym = strlen (flat);
  unsigned char *text = widen (flat, n_sym, 3), *delims = widen ("\nr", 2, 3);
  uint64_t want_off[40];
  const uint64_t n_texts = naive (flat, n_sym, "\nr", 0, want_off);
  CHECK (n_texts == 7 && want_off[2] == 4 && want_off[3] == 7);
  /* \n: none | us\n: s | her: he | s and sh\n: s, s | e sells she\n: s, s, s, she, he | \n: none | on top\n: none */
  const uint64_t want_hits[7] = { 0, 1, 1, 2, 5, 0, 0 };
  uint64_t *off = malloc ((n_texts + 1) * sizeof *off), *hits = malloc (n_texts * sizeof *hits), *out_off = malloc ((n_texts + 1) * sizeof *out_off);
  uint32_t *kept = malloc (n_texts * sizeof *kept);
  const uint64_t kept_symbols = (4 - 1) + (7 - 4) + (16 - 7) + (28 - 16);
  unsigned char *out = malloc (3 * kept_symbols);
  CHECK (off && hits && out_off && kept && out);
  uint64_t nt = 99, nk = 99, total = 99, sym = 99;
  CHECK (acm_internal_cpu_grep_lines (m, text, n_sym, 3, delims, 2, ACM_SPLIT_EVERY, ACM_GREP_MATCHING, &nt, &nk, &total, out, kept_symbols, &sym, n_texts,
                                      off, hits, kept, out_off) == ACM_GPU_OK);
  CHECK (nt == n_texts && memcmp (off, want_off, (n_texts + 1) * sizeof *off) == 0 && memcmp (hits, want_hits, sizeof want_hits) == 0);
  CHECK (nk == 4 && kept[0] == 1 && kept[3] == 4 && total == 9 && sym == kept_symbols && out_off[4] == kept_symbols);
  CHECK (memcmp (out, text + 3 * 1, 3 * kept_symbols) == 0); /* the kept texts are the symbols 1 .. 28, side by side */
  /* no per-text array at all, no output: the numbers alone */
  nt = nk = total = sym = 99;
  CHECK (acm_internal_cpu_grep_lines (m, text, n_sym, 3, delims, 2, ACM_SPLIT_EVERY, ACM_GREP_INVERT, &nt, &nk, &total, NULL, 0, &sym, 0, NULL, NULL, NULL,
                                      NULL) == ACM_GPU_OK);
  CHECK (nt == 7 && nk == 3 && total == 9 && sym == n_sym - kept_symbols);
  /* room for one text too few: only n_texts (the arrays have exactly that room: a write is seen) */
  uint64_t *small_off = malloc (n_texts * sizeof *small_off), *small_hits = malloc ((n_texts - 1) * sizeof *small_hits);
  CHECK (small_off && small_hits);
  nt = 99;
  CHECK (acm_internal_cpu_grep_lines (m, text, n_sym, 3, delims, 2, ACM_SPLIT_EVERY, ACM_GREP_MATCHING, &nt, &nk, &total, out, kept_symbols, &sym,
                                      n_texts - 1, small_off, small_hits, NULL, NULL) == ACM_GPU_E_OVERFLOW);
  CHECK (nt == n_texts);
  /* an output with one symbol too little room: the other overflow, the rest valid */
  unsigned char *small = malloc (3 * (kept_symbols - 1));
  CHECK (small);
  memset (small, '.', 3 * (kept_symbols - 1));
  memset (hits, 0xFF, n_texts * sizeof *hits);
  sym = 99;
  CHECK (acm_internal_cpu_grep_lines (m, text, n_sym, 3, delims, 2, ACM_SPLIT_EVERY, ACM_GREP_MATCHING, &nt, &nk, &total, small, kept_symbols - 1, &sym,
                                      n_texts, off, hits, kept, out_off) == ACM_GPU_E_OVERFLOW);
  CHECK (nt == n_texts && sym == kept_symbols && nk == 4 && memcmp (hits, want_hits, sizeof want_hits) == 0);
  for (uint64_t i = 0; i < 3 * (kept_symbols - 1); i++)
    CHECK (small[i] == '.');
  /* words: RUNS over newline and blank */
  unsigned char *blank = widen ("\n ", 2, 3);
  const uint64_t n_words = naive (flat, n_sym, "\n ", 1, want_off);
  uint64_t *word_off = malloc ((n_words + 1) * sizeof *word_off);
  CHECK (word_off);
  CHECK (acm_internal_cpu_grep_lines (m, text, n_sym, 3, blank, 2, ACM_SPLIT_RUNS, ACM_GREP_MATCHING, &nt, &nk, &total, NULL, 0, NULL, n_words, word_off,
                                      NULL, NULL, NULL) == ACM_GPU_OK);
  CHECK (nt == n_words && memcmp (word_off, want_off, (n_words + 1) * sizeof *word_off) == 0);
  free (word_off), free (blank), free (small), free (small_hits), free (small_off), free (out), free (kept), free (out_off), free (hits), free (off);
  free (delims), free (text);
  acm_release (m);
  for (int k = 0; k < 4; k++)
    free (letters[k]);
  printf ("all checks held\n");
  return 0;
}
