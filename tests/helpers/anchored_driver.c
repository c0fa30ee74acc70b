/* Test-only driver: acm_anchored_records and the caller-loop paths of acm_scan_anchored and acm_lookup
 * (acm_host.c, no HIP) under AddressSanitizer and UBSan.  Every buffer is allocated at its exact size,
 * so that a byte read or written beside it is seen: the last text ends at the last symbol, the record
 * room holds the anchored records and not one more.  The answers are checked against a naive loop
 * written here: a keyword is a prefix of a text when the text's first symbols spell it.  The machine's
 * comparator is memcmp over 3-byte symbols, declared with acm_set_symbol_bytes: what acm_scan_anchored
 * and acm_lookup would run for it are acm_internal_cpu_scan_anchored and acm_internal_cpu_lookup, and
 * those are called here as the public calls call them (which live in the HIP translation unit, which
 * this program does not link).  Built and run by tests/test_anchored_sanitized.py; exits 0 when every
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

#define N_WORDS 7
#define N_TEXTS 16
static const char *const words[N_WORDS] = { "h", "he", "her", "hers", "hershey", "she", "his" };
static const char *const texts[N_TEXTS] = { "", "h", "he", "her", "hers", "hershey", "hersheys", "hex", "she", "xhe", "s", "ushers", "he", "rs", "", "hers" };

/* the letter c as a symbol of 3 bytes */
static unsigned char *
widen3 (const char *word, size_t n) {
  unsigned char *to = malloc (n ? 3 * n : 1);
  CHECK (to);
  for (size_t i = 0; i < n; i++) {
    to[3 * i] = (unsigned char)word[i];
    to[3 * i + 1] = (unsigned char)(word[i] ^ 0x5A);
    to[3 * i + 2] = 7;
  }
  return to;
}

/* ANCHORED by the spelling: for every text the keywords it begins with, by ascending length */
static uint64_t
naive (const uint64_t *off, uint32_t mode, ACMRecord *out, uint32_t *tid, uint64_t *first) {
  uint64_t k = 0;
  for (uint64_t t = 0; t < N_TEXTS; t++) {
    const size_t len = strlen (texts[t]);
    first[t] = k;
    const uint64_t begin = k;
    for (size_t l = 1; l <= len; l++)
      for (uint32_t w = 0; w < N_WORDS; w++) {
        if (strlen (words[w]) != l || memcmp (texts[t], words[w], l) != 0 || (mode == ACM_ANCHORED_WHOLE && l != len))
          continue;
        if (mode == ACM_ANCHORED_LONGEST)
          k = begin; /* a longer one takes the place of the shorter */
        out[k].end_pos = off[t] + l - 1;
        out[k].length = (uint32_t)l;
        out[k].keyword_id = w;
        tid[k] = (uint32_t)t;
        k++;
      }
  }
  first[N_TEXTS] = k;
  return k;
}

static int
cmp3 (const void *a, const void *b, const void *arg) {
  (void)arg;
  return memcmp (a, b, 3);
}

int
main (void) {
  uint64_t *off = malloc ((N_TEXTS + 1) * sizeof *off);
  CHECK (off);
  size_t n = 0;
  for (int t = 0; t < N_TEXTS; t++) {
    off[t] = n;
    n += strlen (texts[t]);
  }
  off[N_TEXTS] = n;
  char *flat = malloc (n + 1);
  CHECK (flat);
  flat[0] = 0;
  for (int t = 0; t < N_TEXTS; t++)
    strcat (flat, texts[t]);
  unsigned char *text = widen3 (flat, n); /* exactly n symbols */

  ACMachine *m = acm_create (cmp3, 0, 0);
  unsigned char *letters[N_WORDS];
  for (int k = 0; k < N_WORDS; k++) {
    const size_t len = strlen (words[k]);
    letters[k] = widen3 (words[k], len);
    const ACState *s = acm_initiate (m);
    for (size_t i = 0; i < len; i++)
      acm_insert_letter_of_keyword (&s, letters[k] + 3 * i);
    acm_insert_end_of_keyword (&s, 0, 0);
  }
  CHECK (acm_set_symbol_bytes (m, 3) == ACM_GPU_OK);

  /* the batch's records, in a room of exactly their number */
  uint64_t n_all = 0;
  CHECK (acm_internal_cpu_scan_batch (m, text, off, N_TEXTS, 3, NULL, NULL, NULL, 0, &n_all) == ACM_GPU_E_OVERFLOW && n_all > 29);
  ACMRecord *all = malloc (n_all * sizeof *all), *want = malloc (n_all * sizeof *want);
  uint32_t *want_tid = malloc (n_all * sizeof *want_tid);
  uint64_t *want_first = malloc ((N_TEXTS + 1) * sizeof *want_first);
  CHECK (all && want && want_tid && want_first);
  CHECK (acm_internal_cpu_scan_batch (m, text, off, N_TEXTS, 3, all, NULL, NULL, n_all, &n_all) == ACM_GPU_OK);

  for (uint32_t mode = ACM_ANCHORED_PREFIXES; mode <= ACM_ANCHORED_WHOLE; mode++) {
    const uint64_t n_want = naive (off, mode, want, want_tid, want_first);
    CHECK (n_want == (mode == ACM_ANCHORED_PREFIXES ? 29u : mode == ACM_ANCHORED_LONGEST ? 10u : 8u));
    /* the sequential pass, in place, with and without the side arrays */
    for (int sides = 0; sides < 2; sides++) {
      ACMRecord *rec = malloc (n_all * sizeof *rec);
      uint32_t *tid = malloc (n_all * sizeof *tid);
      uint64_t *first = malloc ((N_TEXTS + 1) * sizeof *first);
      CHECK (rec && tid && first);
      memcpy (rec, all, n_all * sizeof *rec);
      uint64_t kept = 99;
      CHECK (acm_anchored_records (off, N_TEXTS, mode, rec, n_all, sides ? tid : NULL, sides ? first : NULL, &kept) == ACM_GPU_OK);
      CHECK (kept == n_want && memcmp (rec, want, kept * sizeof *rec) == 0);
      if (sides)
        CHECK (memcmp (tid, want_tid, kept * sizeof *tid) == 0 && memcmp (first, want_first, (N_TEXTS + 1) * sizeof *first) == 0);
      free (first), free (tid), free (rec);
    }
    /* the host path of acm_scan_anchored: room for the anchored records, exactly */
    {
      ACMRecord *rec = malloc (n_want * sizeof *rec);
      uint32_t *tid = malloc (n_want * sizeof *tid);
      uint64_t *first = malloc ((N_TEXTS + 1) * sizeof *first);
      CHECK (rec && tid && first);
      uint64_t found = 99;
      CHECK (acm_internal_cpu_scan_anchored (m, text, off, N_TEXTS, 3, mode, rec, tid, first, n_want, &found) == ACM_GPU_OK);
      CHECK (found == n_want && memcmp (rec, want, found * sizeof *rec) == 0 && memcmp (tid, want_tid, found * sizeof *tid) == 0 &&
             memcmp (first, want_first, (N_TEXTS + 1) * sizeof *first) == 0);
      free (rec), free (tid);
      /* one too little: the need comes back, first[] is complete, nothing is written to the records */
      rec = malloc ((n_want - 1) * sizeof *rec);
      CHECK (rec);
      memset (first, 0xEE, (N_TEXTS + 1) * sizeof *first);
      CHECK (acm_internal_cpu_scan_anchored (m, text, off, N_TEXTS, 3, mode, rec, NULL, first, n_want - 1, &found) == ACM_GPU_E_OVERFLOW);
      CHECK (found == n_want && memcmp (first, want_first, (N_TEXTS + 1) * sizeof *first) == 0);
      free (first), free (rec);
    }
  }

  /* the lookup arrays, each of exactly n_texts entries, all three and one at a time */
  {
    uint32_t *whole = malloc (N_TEXTS * sizeof *whole), *pid = malloc (N_TEXTS * sizeof *pid), *plen = malloc (N_TEXTS * sizeof *plen);
    CHECK (whole && pid && plen);
    CHECK (acm_internal_cpu_lookup (m, text, off, N_TEXTS, 3, whole, pid, plen) == ACM_GPU_OK);
    uint64_t kw = naive (off, ACM_ANCHORED_WHOLE, want, want_tid, want_first);
    for (uint64_t t = 0; t < N_TEXTS; t++) {
      const int hit = want_first[t + 1] > want_first[t];
      CHECK (whole[t] == (hit ? want[want_first[t]].keyword_id : ACM_LOOKUP_NONE));
    }
    CHECK (kw == 8);
    (void)naive (off, ACM_ANCHORED_LONGEST, want, want_tid, want_first);
    for (uint64_t t = 0; t < N_TEXTS; t++) {
      const int hit = want_first[t + 1] > want_first[t];
      CHECK (pid[t] == (hit ? want[want_first[t]].keyword_id : ACM_LOOKUP_NONE) && plen[t] == (hit ? want[want_first[t]].length : 0u));
    }
    CHECK (pid[6] == 4 && plen[6] == 7 && whole[6] == ACM_LOOKUP_NONE); /* "hersheys" */
    uint32_t *only = malloc (N_TEXTS * sizeof *only);
    CHECK (only);
    CHECK (acm_internal_cpu_lookup (m, text, off, N_TEXTS, 3, NULL, NULL, only) == ACM_GPU_OK && memcmp (only, plen, N_TEXTS * sizeof *only) == 0);
    CHECK (acm_internal_cpu_lookup (m, text, off, N_TEXTS, 3, only, NULL, NULL) == ACM_GPU_OK && memcmp (only, whole, N_TEXTS * sizeof *only) == 0);
    CHECK (acm_internal_cpu_lookup (m, text, off, N_TEXTS, 3, NULL, NULL, NULL) == ACM_GPU_E_ARG);
    free (only), free (plen), free (pid), free (whole);
  }

  /* refused, nothing modified */
  {
    ACMRecord *rec = malloc (n_all * sizeof *rec);
    CHECK (rec);
    memcpy (rec, all, n_all * sizeof *rec);
    uint64_t kept = 99;
    CHECK (acm_anchored_records (off, N_TEXTS, 0, rec, n_all, NULL, NULL, &kept) == ACM_GPU_E_ARG);
    CHECK (acm_anchored_records (off, N_TEXTS, 4, rec, n_all, NULL, NULL, &kept) == ACM_GPU_E_ARG);
    CHECK (acm_anchored_records (off, N_TEXTS - 1, ACM_ANCHORED_PREFIXES, rec, n_all, NULL, NULL, &kept) == ACM_GPU_E_ARG); /* the last text's records lie outside */
    uint64_t *bad = malloc ((N_TEXTS + 1) * sizeof *bad);
    CHECK (bad);
    memcpy (bad, off, (N_TEXTS + 1) * sizeof *bad);
    bad[0] = 1;
    CHECK (acm_anchored_records (bad, N_TEXTS, ACM_ANCHORED_PREFIXES, rec, n_all, NULL, NULL, &kept) == ACM_GPU_E_ARG);
    bad[0] = 0;
    bad[7] = bad[8] + 1;
    CHECK (acm_anchored_records (bad, N_TEXTS, ACM_ANCHORED_PREFIXES, rec, n_all, NULL, NULL, &kept) == ACM_GPU_E_ARG);
    free (bad);
    CHECK (memcmp (rec, all, n_all * sizeof *rec) == 0);
    ACMRecord cross = { off[13], 3, 2 }; /* "he" | "rs": `her` across the cut */
    CHECK (acm_anchored_records (off, N_TEXTS, ACM_ANCHORED_PREFIXES, &cross, 1, NULL, NULL, &kept) == ACM_GPU_E_ARG);
    ACMRecord none = { 0, 0, 0 };
    CHECK (acm_anchored_records (off, N_TEXTS, ACM_ANCHORED_PREFIXES, &none, 1, NULL, NULL, &kept) == ACM_GPU_E_ARG);
    /* no text, no record */
    const uint64_t zero[1] = { 0 };
    uint64_t first0[1] = { 99 };
    kept = 99;
    CHECK (acm_anchored_records (zero, 0, ACM_ANCHORED_WHOLE, NULL, 0, NULL, first0, &kept) == ACM_GPU_OK && kept == 0 && first0[0] == 0);
    uint64_t found = 99;
    CHECK (acm_internal_cpu_scan_anchored (m, NULL, zero, 0, 3, ACM_ANCHORED_PREFIXES, NULL, NULL, first0, 0, &found) == ACM_GPU_OK && found == 0);
    free (rec);
  }

  acm_release (m);
  for (int k = 0; k < N_WORDS; k++)
    free (letters[k]);
  free (want_first), free (want_tid), free (want), free (all), free (text), free (flat), free (off);
  printf ("all checks held\n");
  return 0;
}
