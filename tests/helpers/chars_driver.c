/* acm_chars_positions, acm_chars_records (include/acm_chars.h) and what acm_scan_chars runs on the host -- the caller
 * loop, then acm_chars_records (acm_internal_cpu_scan_chars) -- as a program of its own, for AddressSanitizer and UBSan
 * (tests/test_chars_sanitized.py).  Every buffer is allocated at its exact size, so that a read or write one entry
 * beyond it is seen; every expected value is counted here byte by byte, or is the header's table. */
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

static void *
room (size_t bytes, int fill) {
  void *p = malloc (bytes ? bytes : 1);
  CHECK (p);
  memset (p, fill, bytes);
  return p;
}

static int
all_bytes (const void *p, size_t bytes, int fill) {
  for (size_t i = 0; i < bytes; i++)
    if (((const unsigned char *)p)[i] != (unsigned char)fill)
      return 0;
  return 1;
}

/* count (a, b) of the definition, byte by byte */
static uint64_t
count (const unsigned char *t, uint64_t a, uint64_t b, uint32_t unit) {
  uint64_t c = 0;
  for (uint64_t i = a; i < b; i++)
    c += ((t[i] & 0xC0) != 0x80) + (unit == ACM_CHARS_UTF16 && t[i] >= 0xF0);
  return c;
}

/* the text of position p: the last t with offsets[t] <= p */
static uint64_t
text_of (const uint64_t *off, uint64_t n_texts, uint64_t p) {
  uint64_t t = 0;
  for (uint64_t k = 0; k < n_texts; k++)
    if (off[k] <= p)
      t = k;
  return t;
}

static uint32_t lcg_state = 12345;
static uint32_t
lcg (void) {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lcg_state >> 8;
}

/* records and positions of `t` under `off` (may be NULL) against the byte-by-byte definition, in both units */
static void
against_the_definition (const unsigned char *t, uint64_t n, const uint64_t *off, uint64_t n_texts, const ACMRecord *rec, uint64_t n_rec,
                        uint64_t pos_base) {
  for (uint32_t unit = ACM_CHARS_CODEPOINTS; unit <= ACM_CHARS_UTF16; unit++) {
    uint64_t *start = room (n_rec * sizeof *start, 0xEE);
    uint32_t *len = room (n_rec * sizeof *len, 0xEE);
    uint8_t *edge = room (n_rec, 0xEE);
    CHECK (acm_chars_records (t, n, pos_base, off, n_texts, unit, rec, n_rec, start, len, edge) == ACM_GPU_OK);
    for (uint64_t j = 0; j < n_rec; j++) {
      const uint64_t e = rec[j].end_pos - pos_base, s = e + 1 - rec[j].length;
      uint64_t lo = 0, hi = n;
      if (off && n_texts) {
        const uint64_t tx = text_of (off, n_texts, s);
        lo = off[tx];
        hi = off[tx + 1];
      }
      CHECK (start[j] == count (t, lo, s, unit) && len[j] == count (t, s, e + 1, unit));
      const int b0 = s == lo || (t[s] & 0xC0) != 0x80;
      const int b1 = e + 1 == hi || e + 1 >= n || (t[e + 1] & 0xC0) != 0x80;
      CHECK (edge[j] == (uint8_t)((b0 ? 0 : 1) | (b1 ? 0 : 2)));
    }
    free (edge), free (len), free (start);
    uint64_t *pos = malloc ((n + 1) * sizeof *pos), *out = room ((n + 1) * sizeof *out, 0xEE);
    CHECK (pos);
    for (uint64_t p = 0; p <= n; p++)
      pos[p] = n - p; /* any order */
    CHECK (acm_chars_positions (t, n, off, n_texts, unit, pos, n + 1, out) == ACM_GPU_OK);
    for (uint64_t p = 0; p <= n; p++)
      CHECK (out[p] == count (t, off && n_texts ? off[text_of (off, n_texts, pos[p])] : 0, pos[p], unit));
    free (out), free (pos);
  }
}

/* equal modulo 3, and no order (a < b < c < a): no class table exists for it, the loop is the only path */
static int
cyclic_cmp (const void *a, const void *b, const void *arg) {
  (void)arg;
  const unsigned x = *(const unsigned char *)a % 3u, y = *(const unsigned char *)b % 3u;
  if (x == y)
    return 0;
  return (x + 1) % 3 == y ? -1 : 1;
}

int
main (void) {
  /* the header's example, number for number */
  static const unsigned char example[18] = { 0x61, 0xc3, 0xa9, 0xe2, 0x82, 0xac, 0xf0, 0x9f, 0x98, 0x80, 0x20, 0xc3, 0xa9, 0xf0, 0x9f, 0x98, 0x80, 0x61 };
  static const ACMRecord table[10] = { { 0, 1, 3 }, { 2, 2, 0 }, { 2, 1, 4 }, { 9, 7, 1 }, { 9, 4, 2 }, { 10, 4, 5 }, { 12, 2, 0 }, { 12, 1, 4 }, { 16, 4, 2 }, { 17, 1, 3 } };
  static const uint64_t want_start[2][10] = { { 0, 1, 2, 2, 3, 4, 5, 6, 6, 7 }, { 0, 1, 2, 2, 3, 5, 6, 7, 7, 9 } };
  static const uint32_t want_len[2][10] = { { 1, 1, 0, 2, 1, 1, 1, 0, 1, 1 }, { 1, 1, 0, 3, 2, 1, 1, 0, 2, 1 } };
  static const uint8_t want_edge[10] = { 0, 0, 1, 0, 0, 1, 0, 1, 0, 0 };
  unsigned char *text = exact (example, 18);
  ACMRecord *rec = exact (table, sizeof table);
  uint64_t *start = room (10 * sizeof *start, 0xEE);
  uint32_t *len = room (10 * sizeof *len, 0xEE);
  uint8_t *edge = room (10, 0xEE);
  for (uint32_t unit = 1; unit <= 2; unit++) {
    CHECK (acm_chars_records (text, 18, 0, NULL, 0, unit, rec, 10, start, len, edge) == ACM_GPU_OK);
    CHECK (memcmp (start, want_start[unit - 1], sizeof want_start[0]) == 0 && memcmp (len, want_len[unit - 1], sizeof want_len[0]) == 0 &&
           memcmp (edge, want_edge, 10) == 0);
    uint64_t whole = 99, end = 18;
    CHECK (acm_chars_positions (text, 18, NULL, 0, unit, &end, 1, &whole) == ACM_GPU_OK && whole == (unit == 1 ? 8u : 10u));
  }
  against_the_definition (text, 18, NULL, 0, rec, 10, 0);
  /* each output alone; all three NULL, a unit that is none, broken offsets and records: nothing is written */
  memset (start, 0xEE, 10 * sizeof *start), memset (len, 0xEE, 10 * sizeof *len), memset (edge, 0xEE, 10);
  CHECK (acm_chars_records (text, 18, 0, NULL, 0, 1, rec, 10, NULL, NULL, NULL) == ACM_GPU_E_ARG);
  CHECK (acm_chars_records (text, 18, 0, NULL, 0, 0, rec, 10, start, len, edge) == ACM_GPU_E_ARG);
  CHECK (acm_chars_records (text, 18, 0, NULL, 0, 3, rec, 10, start, len, edge) == ACM_GPU_E_ARG);
  uint64_t *bad_off = exact ((uint64_t[]){ 0, 9, 8, 18 }, 4 * sizeof (uint64_t));
  CHECK (acm_chars_records (text, 18, 0, bad_off, 3, 1, rec, 10, start, len, edge) == ACM_GPU_E_ARG);
  bad_off[1] = 8, bad_off[3] = 17;
  CHECK (acm_chars_records (text, 18, 0, bad_off, 3, 1, rec, 10, start, len, edge) == ACM_GPU_E_ARG);
  bad_off[3] = 18, bad_off[0] = 1;
  CHECK (acm_chars_records (text, 18, 0, bad_off, 3, 1, rec, 10, start, len, edge) == ACM_GPU_E_ARG);
  CHECK (acm_chars_records (text, 18, 1, NULL, 0, 1, rec, 10, start, len, edge) == ACM_GPU_E_ARG); /* (the first record ends in front of pos_base) */
  static const ACMRecord broken[3] = { { 18, 1, 0 }, { 5, 0, 0 }, { 3, 5, 0 } };
  for (int k = 0; k < 3; k++) {
    ACMRecord *one = exact (&broken[k], sizeof broken[k]);
    CHECK (acm_chars_records (text, 18, 0, NULL, 0, 1, one, 1, start, len, edge) == ACM_GPU_E_ARG);
    free (one);
  }
  uint64_t beyond = 19, out = 0xEEEEEEEEEEEEEEEEull;
  CHECK (acm_chars_positions (text, 18, NULL, 0, 1, &beyond, 1, &out) == ACM_GPU_E_ARG && out == 0xEEEEEEEEEEEEEEEEull);
  CHECK (all_bytes (start, 10 * sizeof *start, 0xEE) && all_bytes (len, 10 * sizeof *len, 0xEE) && all_bytes (edge, 10, 0xEE));
  CHECK (acm_chars_records (text, 18, 0, NULL, 0, 2, rec, 10, NULL, len, NULL) == ACM_GPU_OK && memcmp (len, want_len[1], sizeof want_len[0]) == 0);
  CHECK (all_bytes (start, 10 * sizeof *start, 0xEE) && all_bytes (edge, 10, 0xEE));
  /* no byte at all: one empty text, with and without offsets */
  uint64_t *zero_off = exact ((uint64_t[]){ 0, 0, 0 }, 3 * sizeof (uint64_t)), p0 = 0;
  out = 99;
  CHECK (acm_chars_positions (NULL, 0, NULL, 0, 1, &p0, 1, &out) == ACM_GPU_OK && out == 0);
  out = 99;
  CHECK (acm_chars_positions (NULL, 0, zero_off, 2, 2, &p0, 1, &out) == ACM_GPU_OK && out == 0);
  out = 99;
  CHECK (acm_chars_positions (NULL, 0, zero_off, 0, 2, &p0, 1, &out) == ACM_GPU_OK && out == 0);
  CHECK (acm_chars_records (NULL, 0, 0, NULL, 0, 1, NULL, 0, start, len, edge) == ACM_GPU_OK);
  /* random bytes from a small set of leads, continuations and ASCII: every record of up to 9 bytes at every start of a
   * 301-byte buffer, under cuts with empty texts first, last and adjacent, and under a pos_base with bit 63 set */
  static const unsigned char bytes[8] = { 0x61, 0x20, 0xc3, 0xa9, 0xe2, 0x82, 0xf0, 0x9f };
  const uint64_t n = 301;
  unsigned char *t = malloc (n);
  CHECK (t);
  for (uint64_t i = 0; i < n; i++)
    t[i] = bytes[lcg () % 8];
  uint64_t n_rec = 0;
  for (uint64_t s = 0; s < n; s++)
    for (uint32_t l = 1; l <= 9 && s + l <= n; l++)
      n_rec++;
  ACMRecord *every = malloc (n_rec * sizeof *every);
  CHECK (every);
  const uint64_t base = (1ull << 63) + 9;
  uint64_t at = 0;
  for (uint64_t s = 0; s < n; s++)
    for (uint32_t l = 1; l <= 9 && s + l <= n; l++)
      every[at++] = (ACMRecord){ base + s + l - 1, l, (uint32_t)(lcg () % 7) };
  for (uint64_t j = n_rec - 1; j > 0; j--) { /* any order */
    const uint64_t k = lcg () % (j + 1);
    const ACMRecord x = every[j];
    every[j] = every[k];
    every[k] = x;
  }
  uint64_t *off = exact ((uint64_t[]){ 0, 0, 0, 17, 64, 64, 65, 128, 200, 200, 200, 300, 301, 301, 301 }, 15 * sizeof (uint64_t));
  against_the_definition (t, n, NULL, 0, every, n_rec, base);
  against_the_definition (t, n, off, 14, every, n_rec, base);
  /* what acm_scan_chars runs on the host: the caller loop of a machine no GPU path takes, then the map */
  ACMachine *m = acm_create (cyclic_cmp, 0, 0);
  static const unsigned char kw[3][3] = { { 0xc3, 0xa9, 0 }, { 0x61, 0, 0 }, { 0xf0, 0x9f, 0x82 } };
  static const size_t kw_len[3] = { 2, 1, 3 };
  unsigned char *letters[3];
  for (int k = 0; k < 3; k++) {
    letters[k] = exact (kw[k], kw_len[k]);
    const ACState *s = acm_initiate (m);
    for (size_t i = 0; i < kw_len[k]; i++)
      acm_insert_letter_of_keyword (&s, letters[k] + i);
    acm_insert_end_of_keyword (&s, 0, 0);
  }
  CHECK (acm_set_symbol_bytes (m, 1) == ACM_GPU_OK);
  uint64_t found = 0, needed = 0;
  CHECK (acm_internal_cpu_scan_chars (m, t, n, 1, ACM_CHARS_UTF16, NULL, NULL, NULL, edge, 0, &needed) == ACM_GPU_E_OVERFLOW && needed > 10);
  ACMRecord *got = room (needed * sizeof *got, 0xEE);
  uint64_t *g_start = room (needed * sizeof *g_start, 0xEE);
  uint32_t *g_len = room (needed * sizeof *g_len, 0xEE);
  uint8_t *g_edge = room (needed, 0xEE);
  CHECK (acm_internal_cpu_scan_chars (m, t, n, 1, ACM_CHARS_UTF16, got, g_start, g_len, g_edge, needed - 1, &found) == ACM_GPU_E_OVERFLOW && found == needed);
  CHECK (acm_internal_cpu_scan_chars (m, t, n, 1, ACM_CHARS_UTF16, got, g_start, g_len, g_edge, needed, &found) == ACM_GPU_OK && found == needed);
  for (uint64_t j = 0; j < found; j++) {
    const uint64_t e = got[j].end_pos, s = e + 1 - got[j].length;
    CHECK (e < n && got[j].keyword_id < 3 && got[j].length == kw_len[got[j].keyword_id]);
    CHECK (g_start[j] == count (t, 0, s, ACM_CHARS_UTF16) && g_len[j] == count (t, s, e + 1, ACM_CHARS_UTF16) && g_edge[j] <= 3);
  }
  CHECK (acm_internal_cpu_scan_chars (m, t, n, 2, ACM_CHARS_UTF16, got, g_start, g_len, g_edge, needed, &found) == ACM_GPU_E_ARG); /* not bytes */
  CHECK (acm_internal_cpu_scan_chars (m, t, n, 1, 0, got, g_start, g_len, g_edge, needed, &found) == ACM_GPU_E_ARG);
  CHECK (acm_internal_cpu_scan_chars (m, t, n, 1, 1, got, NULL, NULL, NULL, needed, &found) == ACM_GPU_E_ARG);
  free (g_edge), free (g_len), free (g_start), free (got);
  acm_release (m);
  for (int k = 0; k < 3; k++)
    free (letters[k]);
  free (off), free (every), free (t), free (zero_off), free (bad_off), free (edge), free (len), free (start), free (rec), free (text);
  printf ("all checks held\n");
  return 0;
}
