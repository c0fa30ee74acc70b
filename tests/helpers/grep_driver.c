/* Test-only driver: acm_grep_gather and acm_grep's host path (acm_host.c, no HIP) under
 * AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte read or
 * written beside it is seen.  The machine's comparator is memcmp over 3-byte symbols, declared with
 * acm_set_symbol_bytes: what acm_grep runs for it is the caller loop on the host.  The loop and the
 * gather are called on their own, and then acm_internal_cpu_grep, the very function acm_grep calls
 * for such a machine (acm_grep itself lives in the HIP translation unit, which this program does not
 * link).  Built and run by tests/test_grep_sanitized.py; exits 0 when every check held. */
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

int
main (void) {
  /* {he, she, hers, s} over the texts "", "us", "hers and sh", "e sells she", "", "on top", "": "us|hers" and "sh|e"
   * cut a keyword, "on top" has no match, the empty texts sit at the front, in the middle and at the end */
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
  const uint64_t cuts[8] = { 0, 0, 2, 13, 24, 24, 30, 30 };
  const uint64_t n_texts = 7, n_sym = 30;
  CHECK (strlen (flat) == n_sym);
  unsigned char *text = malloc (3 * n_sym);
  CHECK (text);
  sym3 (text, flat, n_sym);
  uint64_t *off = exact (cuts, sizeof cuts);
  uint64_t *hits = malloc (n_texts * sizeof *hits);
  CHECK (hits);
  CHECK (acm_internal_cpu_grep_hits (m, text, off, n_texts, 3, hits) == ACM_GPU_OK);
  /* us: s | hers and sh: he, hers, s, s | e sells she: s, s, s, she, he | on top: none */
  const uint64_t want_hits[7] = { 0, 1, 4, 5, 0, 0, 0 };
  CHECK (memcmp (hits, want_hits, sizeof want_hits) == 0);

  /* MATCHING: texts 1, 2, 3 */
  uint32_t *kept = malloc (n_texts * sizeof *kept);
  uint64_t *out_off = malloc ((n_texts + 1) * sizeof *out_off);
  unsigned char *out = malloc (3 * 24);
  CHECK (kept && out_off && out);
  uint64_t n_kept = 99, out_symbols = 99;
  CHECK (acm_grep_gather (text, 3, off, n_texts, hits, ACM_GREP_MATCHING, kept, &n_kept, out, 24, out_off, &out_symbols) == ACM_GPU_OK);
  CHECK (n_kept == 3 && kept[0] == 1 && kept[1] == 2 && kept[2] == 3);
  CHECK (out_symbols == 24 && out_off[0] == 0 && out_off[1] == 2 && out_off[2] == 13 && out_off[3] == 24);
  CHECK (memcmp (out, text, 3 * 24) == 0);
  /* one symbol too little room: the need, nothing written, kept and the offsets all the same */
  unsigned char *small = malloc (3 * 23);
  CHECK (small);
  memset (small, '.', 3 * 23);
  memset (kept, 0xFF, n_texts * sizeof *kept);
  n_kept = out_symbols = 99;
  CHECK (acm_grep_gather (text, 3, off, n_texts, hits, ACM_GREP_MATCHING, kept, &n_kept, small, 23, out_off, &out_symbols) == ACM_GPU_E_OVERFLOW);
  CHECK (out_symbols == 24 && n_kept == 3 && kept[2] == 3 && out_off[3] == 24);
  for (int i = 0; i < 3 * 23; i++)
    CHECK (small[i] == '.');
  /* INVERT: the empty texts and "on top"; the output buffer has exactly the 6 symbols */
  unsigned char *inv = malloc (3 * 6);
  CHECK (inv);
  CHECK (acm_grep_gather (text, 3, off, n_texts, hits, ACM_GREP_INVERT, kept, &n_kept, inv, 6, out_off, &out_symbols) == ACM_GPU_OK);
  CHECK (n_kept == 4 && kept[0] == 0 && kept[1] == 4 && kept[2] == 5 && kept[3] == 6);
  CHECK (out_symbols == 6 && out_off[0] == 0 && out_off[1] == 0 && out_off[2] == 0 && out_off[3] == 6 && out_off[4] == 6);
  CHECK (memcmp (inv, text + 3 * 24, 3 * 6) == 0);
  /* no output arrays at all; no text at all; offsets that decrease */
  CHECK (acm_grep_gather (text, 3, off, n_texts, hits, ACM_GREP_MATCHING, NULL, &n_kept, NULL, 0, NULL, NULL) == ACM_GPU_OK && n_kept == 3);
  uint64_t *zero = exact ((uint64_t[]){ 0 }, sizeof (uint64_t));
  CHECK (acm_grep_gather (NULL, 3, zero, 0, NULL, ACM_GREP_INVERT, NULL, &n_kept, NULL, 0, NULL, &out_symbols) == ACM_GPU_OK);
  CHECK (n_kept == 0 && out_symbols == 0);
  /* what acm_grep runs on the host, with hit counters of its own: the loop, the total, the gather */
  uint64_t total = 99;
  n_kept = out_symbols = 99;
  memset (out, 0, 3 * 24);
  CHECK (acm_internal_cpu_grep (m, text, off, n_texts, 3, ACM_GREP_MATCHING, NULL, kept, &n_kept, &total, out, 24, out_off, &out_symbols) == ACM_GPU_OK);
  CHECK (n_kept == 3 && kept[0] == 1 && kept[2] == 3 && total == 10 && out_symbols == 24 && out_off[3] == 24 && memcmp (out, text, 3 * 24) == 0);
  /* one text of 3000 x "s": 3000 matches, counted into the caller's one counter */
  unsigned char *big = malloc (3 * 3000);
  uint64_t *big_off = exact ((uint64_t[]){ 0, 3000 }, 2 * sizeof (uint64_t)), *big_hits = malloc (sizeof *big_hits);
  CHECK (big && big_hits);
  for (int i = 0; i < 3000; i++)
    sym3 (big + 3 * i, "s", 1);
  CHECK (acm_internal_cpu_grep (m, big, big_off, 1, 3, ACM_GREP_MATCHING, big_hits, NULL, &n_kept, &total, NULL, 0, NULL, &out_symbols) == ACM_GPU_OK);
  CHECK (n_kept == 1 && total == 3000 && big_hits[0] == 3000 && out_symbols == 3000);
  free (big_hits), free (big_off), free (big);
  off[2] = 14;
  CHECK (acm_grep_gather (text, 3, off, n_texts, hits, ACM_GREP_MATCHING, kept, &n_kept, out, 24, out_off, &out_symbols) == ACM_GPU_E_ARG);
  free (zero), free (inv), free (small), free (out), free (out_off), free (kept), free (hits), free (off), free (text);
  acm_release (m);
  for (int k = 0; k < 4; k++)
    free (letters[k]);
  printf ("all checks held\n");
  return 0;
}
