/* Test-only driver: acm_templates_check, acm_templates_split and acm_templates_records (acm_host.c, no HIP) under
 * AddressSanitizer and UBSan.  Every buffer is allocated at its exact size, so that a byte read or written beside
 * it is seen.  The templates are written in a notation of this file (a lower-case letter or a blank is a literal,
 * `.` ANY, `D` the digits, `V` the vowels, `N` everything but the vowels, `E` the negated empty class), cut here by
 * acm_templates_split, whose pieces are checked against the definition of the cut; the records are made here by
 * a naive loop over the text (the canonical order), and the pass is checked against a naive window scan written
 * here.  Built and run by tests/test_templates_sanitized.py; exits 0 when every check held. */
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

static const char *const TEMPLATES[] = { "id-DDD", "abVcdNef", "D-D.D-D", "xEy", "V" "ab" };
static const uint32_t BUDGET[] = { 0, 2, 1, 1, 0 };
enum { N_TEMPLATES = 5, MOST_PIECES = 16, N_CLASSES = 4 };
/* classes 0 to 3: D, V, N, E */
static const unsigned char RANGES[] = { '0', '9', 'a', 'a', 'e', 'e', 'i', 'i', 'o', 'o', 'u', 'u', 'a', 'a', 'e', 'e', 'i', 'i', 'o', 'o', 'u', 'u' };
static const uint64_t CLS_PTR[N_CLASSES + 1] = { 0, 1, 6, 11, 11 };
static const uint32_t CLS_FLAGS[N_CLASSES] = { 0, 0, ACM_TEMPLATE_NEGATED, ACM_TEMPLATE_NEGATED };

static int
literal (char c) {
  return (c >= 'a' && c <= 'z') || c == ' ' || c == '-';
}

static int
vowel (char c) {
  return c == 'a' || c == 'e' || c == 'i' || c == 'o' || c == 'u';
}

/* whether the cell written `c` accepts the symbol x */
static int
accepts (char c, char x) {
  switch (c) {
  case '.':
  case 'E': return 1;
  case 'D': return x >= '0' && x <= '9';
  case 'V': return vowel (x);
  case 'N': return !vowel (x);
  default: return c == x;
  }
}

static uint32_t
cell_word (char c) {
  return literal (c) ? ACM_TEMPLATE_LITERAL : c == '.' ? ACM_TEMPLATE_ANY : c == 'D' ? 0u : c == 'V' ? 1u : c == 'N' ? 2u : 3u;
}

/* the set of a run: the distinct pieces are the keywords, in order of first appearance */
struct set {
  char *spell;
  uint32_t *cells, *k, *cls_flags;
  uint64_t *spell_off, *tgt_ptr, *cls_ptr;
  unsigned char *ranges;
  ACMPatternTerm *terms;
  char words[MOST_PIECES][16];
  int n_words;
  uint64_t n_terms;
  ACMTemplateSpec spec;
};

/* pieces of q cells on the literal runs of a template, by the definition */
static uint64_t
pieces_of (const char *t, uint64_t q) {
  uint64_t pieces = 0, run = 0;
  for (size_t i = 0;; i++) {
    if (t[i] && literal (t[i])) {
      run++;
      continue;
    }
    pieces += run / q;
    run = 0;
    if (!t[i])
      return pieces;
  }
}

static void
make_set (struct set *s) {
  char spell[64];
  uint32_t cells[64];
  uint64_t spell_off[N_TEMPLATES + 1] = { 0 }, tgt_ptr[N_TEMPLATES + 1] = { 0 };
  ACMPatternTerm terms[MOST_PIECES];
  s->n_words = 0;
  s->n_terms = 0;
  for (int w = 0; w < N_TEMPLATES; w++) {
    const uint64_t L = strlen (TEMPLATES[w]);
    for (uint64_t i = 0; i < L; i++) {
      spell[spell_off[w] + i] = literal (TEMPLATES[w][i]) ? TEMPLATES[w][i] : 0;
      cells[spell_off[w] + i] = cell_word (TEMPLATES[w][i]);
    }
    spell_off[w + 1] = spell_off[w] + L;
    uint32_t *mine = exact (cells + spell_off[w], L * sizeof *mine);
    uint64_t q = 1;
    while (pieces_of (TEMPLATES[w], q + 1) >= BUDGET[w] + 1)
      q++;
    uint64_t behind = 0;
    for (uint32_t j = 0; j <= BUDGET[w]; j++) {
      uint64_t o = 0, n = 0;
      CHECK (acm_templates_split (mine, L, BUDGET[w], j, &o, &n) == ACM_GPU_OK);
      CHECK (n == q && o >= behind && o + n <= L); /* pieces of the largest length, left to right, disjoint */
      for (uint64_t i = o; i < o + n; i++)
        CHECK (literal (TEMPLATES[w][i]));
      behind = o + n;
      char piece[16] = { 0 };
      memcpy (piece, TEMPLATES[w] + o, n);
      int id = 0;
      while (id < s->n_words && strcmp (s->words[id], piece))
        id++;
      if (id == s->n_words)
        strcpy (s->words[s->n_words++], piece);
      terms[s->n_terms++] = (ACMPatternTerm){ (uint32_t)id, (uint32_t)o, (uint32_t)n };
    }
    uint64_t o = 0, n = 0;
    CHECK (acm_templates_split (mine, L, BUDGET[w], BUDGET[w] + 1, &o, &n) == ACM_GPU_E_ARG);
    CHECK (acm_templates_split (mine, L, (uint32_t)L, 0, &o, &n) == ACM_GPU_E_ARG); /* (k + 1 pieces need more literal cells than the template has cells) */
    free (mine);
    tgt_ptr[w + 1] = s->n_terms;
  }
  s->spell = exact (spell, spell_off[N_TEMPLATES]);
  s->cells = exact (cells, spell_off[N_TEMPLATES] * sizeof *cells);
  s->spell_off = exact (spell_off, sizeof spell_off);
  s->tgt_ptr = exact (tgt_ptr, sizeof tgt_ptr);
  s->k = exact (BUDGET, sizeof BUDGET);
  s->terms = exact (terms, s->n_terms * sizeof *terms);
  s->ranges = exact (RANGES, sizeof RANGES);
  s->cls_ptr = exact (CLS_PTR, sizeof CLS_PTR);
  s->cls_flags = exact (CLS_FLAGS, sizeof CLS_FLAGS);
  s->spec = (ACMTemplateSpec){ s->spell, s->spell_off, s->cells, s->k, s->terms, s->tgt_ptr, N_TEMPLATES, s->ranges, s->cls_ptr, s->cls_flags, N_CLASSES };
}

static void
free_set (struct set *s) {
  free (s->spell);
  free (s->cells);
  free (s->spell_off);
  free (s->tgt_ptr);
  free (s->k);
  free (s->terms);
  free (s->ranges);
  free (s->cls_ptr);
  free (s->cls_flags);
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

/* every window of every template within its budget inside one text, by end ascending, longest first, template ascending */
static uint64_t
naive_windows (const char *text, size_t n, const uint64_t *off, uint64_t n_texts, uint64_t pos_base, ACMRecord *out, uint32_t *dist) {
  uint64_t k = 0;
  const uint64_t whole[2] = { 0, n };
  if (!off) {
    off = whole;
    n_texts = 1;
  }
  for (size_t e = 0; e < n; e++)
    for (size_t len = 16; len >= 1; len--)
      for (int w = 0; w < N_TEMPLATES; w++) {
        if (strlen (TEMPLATES[w]) != len || len > e + 1)
          continue;
        const size_t S = e + 1 - len;
        int inside = 0;
        for (uint64_t t = 0; t < n_texts; t++)
          inside = inside || (off[t] <= S && S + len <= off[t + 1]);
        uint32_t d = 0;
        for (size_t i = 0; i < len; i++)
          d += !accepts (TEMPLATES[w][i], text[S + i]);
        if (inside && d <= BUDGET[w]) {
          if (out) {
            out[k] = (ACMRecord){ pos_base + e, (uint32_t)len, (uint32_t)w };
            dist[k] = d;
          }
          k++;
        }
      }
  return k;
}

static void
run (const char *text_literal, const uint64_t *off_in, uint64_t n_texts, uint64_t pos_base, uint64_t least) {
  struct set s;
  make_set (&s);
  const size_t n = strlen (text_literal);
  char *text = exact (text_literal, n);
  uint64_t *off = off_in ? exact (off_in, (n_texts + 1) * sizeof *off) : NULL;
  uint64_t n_rec = 0, found = 0;
  ACMRecord *rec = naive_records (text, n, &s, pos_base, &n_rec);
  CHECK (acm_templates_check (&s.spec, 1, (uint64_t)s.n_words) == ACM_GPU_OK);
  CHECK (acm_templates_check (&s.spec, 1, (uint64_t)s.n_words - 1) == ACM_GPU_E_ARG);
  const uint64_t want_n = naive_windows (text, n, off, n_texts, pos_base, NULL, NULL);
  CHECK (want_n >= least);
  ACMRecord *want = malloc ((want_n ? want_n : 1) * sizeof *want), *out = malloc ((want_n ? want_n : 1) * sizeof *out);
  uint32_t *want_d = malloc ((want_n ? want_n : 1) * sizeof *want_d), *dist = malloc ((want_n ? want_n : 1) * sizeof *dist);
  CHECK (want && out && want_d && dist);
  naive_windows (text, n, off, n_texts, pos_base, want, want_d);
  /* count only; one entry too few; the exact room without and with distances */
  CHECK (acm_templates_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, &s.spec, (uint64_t)s.n_words, NULL, NULL, 0, &found) == ACM_GPU_OK);
  CHECK (found == want_n);
  if (want_n) {
    CHECK (acm_templates_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, &s.spec, (uint64_t)s.n_words, out, dist, want_n - 1, &found) ==
           ACM_GPU_E_OVERFLOW);
    CHECK (found == want_n);
  }
  CHECK (acm_templates_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, &s.spec, (uint64_t)s.n_words, out, NULL, want_n, &found) == ACM_GPU_OK);
  CHECK (acm_templates_records (rec, n_rec, text, 1, n, pos_base, off, n_texts, &s.spec, (uint64_t)s.n_words, out, dist, want_n, &found) == ACM_GPU_OK);
  CHECK (found == want_n);
  for (uint64_t i = 0; i < want_n; i++)
    CHECK (out[i].end_pos == want[i].end_pos && out[i].length == want[i].length && out[i].keyword_id == want[i].keyword_id && dist[i] == want_d[i]);
  free (want);
  free (out);
  free (want_d);
  free (dist);
  free (rec);
  free (off);
  free (text);
  free_set (&s);
}

/* the argument errors that read arrays: each on arrays of the exact size */
static void
refusals (void) {
  struct set s;
  make_set (&s);
  ACMTemplateSpec t = s.spec;
  uint32_t *cells = exact (s.cells, s.spell_off[N_TEMPLATES] * sizeof *cells);
  t.cells = cells;
  cells[3] = N_CLASSES; /* a class id that is no class */
  CHECK (acm_templates_check (&t, 1, (uint64_t)s.n_words) == ACM_GPU_E_ARG);
  cells[3] = 0;
  cells[0] = 0; /* the first term of template 0 stands on `id-`: now over a class cell */
  CHECK (acm_templates_check (&t, 1, (uint64_t)s.n_words) == ACM_GPU_E_ARG);
  free (cells);
  t = s.spec;
  unsigned char *ranges = exact (RANGES, sizeof RANGES);
  ranges[0] = '9';
  ranges[1] = '0'; /* lo > hi */
  t.ranges = ranges;
  CHECK (acm_templates_check (&t, 1, (uint64_t)s.n_words) == ACM_GPU_E_ARG);
  free (ranges);
  t = s.spec;
  const uint64_t many[2] = { 0, 17 };
  uint64_t *cls_ptr = exact (many, sizeof many);
  t.cls_ptr = cls_ptr;
  t.n_classes = 1; /* 17 ranges: refused before ranges[] is read that far */
  CHECK (acm_templates_check (&t, 1, (uint64_t)s.n_words) == ACM_GPU_E_ARG);
  free (cls_ptr);
  t = s.spec;
  t.n_classes = 0xFFFFFFFEull;
  CHECK (acm_templates_check (&t, 1, (uint64_t)s.n_words) == ACM_GPU_E_ARG);
  CHECK (acm_templates_check (&s.spec, 3, (uint64_t)s.n_words) == ACM_GPU_E_ARG);
  CHECK (acm_templates_check (NULL, 1, 0) == ACM_GPU_E_ARG);
  uint64_t found = 0;
  CHECK (acm_templates_records (NULL, 0, NULL, 1, 0, 0, NULL, 0, NULL, 0, NULL, NULL, 0, &found) == ACM_GPU_E_ARG);
  free_set (&s);
}

int
main (void) {
  const char *text = "id-123 id-12x abecdxef abXcdaeX 1-2x3-4 1-2-3-4 9-9 8-x78-9 xay xxy eab id-999abicdtef 00000";
  run (text, NULL, 0, 0, 12);
  run (text, NULL, 0, 1ull << 40, 12);
  const uint64_t cuts[] = { 0, 0, 4, 30, 30, 61, strlen (text) };
  run (text, cuts, 6, 7, 6);
  run ("", NULL, 0, 0, 0);
  const uint64_t none[] = { 0, 0 };
  run ("", none, 1, 0, 0);
  run ("ab", NULL, 0, 0, 0);
  refusals ();
  printf ("all checks held\n");
  return 0;
}
