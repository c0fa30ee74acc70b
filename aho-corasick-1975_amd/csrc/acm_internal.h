/* Internal interface between the host trie (acm_host.c), the flattener (acm_flat.c) and the
 * device side (acm_gpu.hip).  Not installed. */
#ifndef ACM_INTERNAL_H
#define ACM_INTERNAL_H

#include "acm.h"
#include "acm_gpu.h"
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Goto edges of a state: children ordered by the machine comparator on ->letter.  One block that
 * is replaced (never freed before acm_release) when it outgrows its capacity, so that a reader
 * that runs beside an insertion (acm_match is not locked, as in the reference: README.md:364)
 * never touches freed memory; `kver` of the owning state is a sequence lock around in-place
 * insertions (odd while one is under way). */
struct _ac_kidvec {
  uint32_t n, cap;
  struct _ac_state *v[];
};
/* for code that holds the machine lock (writers, the flattener) */
#define ACM_NKIDS(s) ((s)->kids ? (s)->kids->n : 0u)
#define ACM_KID(s, i) ((s)->kids->v[i])

struct _ac_state {
  ACMachine *machine;
  struct _ac_state *parent; /* reference: previous.state, aho_corasick.c:49-52 */
  void *letter;             /* symbol on the edge parent -> this, as handed in by the caller */
  struct _ac_state *fail;   /* f(s); NULL for the root only */
  struct _ac_kidvec *kids;  /* goto edges (NULL: none) */
  struct _ac_state **inv;   /* inverse failure set { x : f(x) == this }, unordered; writers only */
  uint32_t kver;            /* sequence lock of `kids` */
  uint32_t ninv, capinv;
  uint32_t inv_slot;        /* position of this state inside fail->inv (O(1) removal) */
  uint32_t depth;
  uint32_t nb_outputs;      /* keywords ending here = terminal + nb_outputs(fail) */
  uint32_t rank;            /* keyword_id when terminal */
  uint32_t id;              /* creation order, printed by acm_print */
  int terminal;
  void *value;
  void (*value_dtor) (void *);
};

/* dictionary generation counter: bumped whenever a node or a keyword is added; a cached device
 * plan built at another generation is stale. */
uint64_t acm_internal_generation (const ACMachine *m);
ACState *acm_internal_root (const ACMachine *m);
uint32_t acm_internal_nb_states (const ACMachine *m);
/* 0 if the machine uses ACM_CMP_DEFAULT over 1, 2 or 4 byte symbols, else ACM_GPU_E_INELIGIBLE */
int acm_internal_symbol_bytes (const ACMachine *m, uint32_t *sym_bytes);
void acm_internal_comparator (const ACMachine *m, CMP_TYPE *cmp, void **cmp_arg);
/* acm_set_symbol_bytes' value (0: none); the caller loop on the host for machines the GPU cannot take; acm_scan_path's value */
uint32_t acm_internal_declared_symbol_bytes (const ACMachine *m);
int acm_internal_cpu_scan (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records, uint64_t capacity,
                           uint64_t *n_found);
/* the same loop from the root on every text of a batch (acm_scan_batch); offsets[] already checked */
int acm_internal_cpu_scan_batch (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, ACMRecord *records,
                                 uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found);
/* the same loop continued from *cursor (acm_scan_from); *cursor is unchanged unless the call returns ACM_GPU_OK */
int acm_internal_cpu_scan_from (ACMachine *m, const ACState **cursor, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records,
                                uint64_t capacity, uint64_t *n_found);
/* the same loop, counting per keyword instead of recording (acm_tally): tally[keyword_id] += 1 per match, *total (may be
 * NULL) = their number; ACM_GPU_E_ARG, with nothing counted, when n_keywords is below the machine's number of keywords */
int acm_internal_cpu_tally (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t *tally, uint64_t n_keywords,
                            uint64_t *total);
/* the same loop from the root on every text of a batch, counting per text instead of recording (acm_grep): hits[t] = the
 * number of matches of text t; offsets[] already checked */
int acm_internal_cpu_grep_hits (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint64_t *hits);
/* The host paths of the calls that give their caller no record room: arguments as the public call's (include/acm_gpu.h)
 * with the symbol size behind the text; the public call has checked them.  The record room is the call's own and grown once. */
int acm_internal_cpu_select (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records, uint64_t capacity,
                             uint64_t *n_found);
int acm_internal_cpu_segment (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint32_t *cost, uint64_t n_keywords,
                              uint32_t gap_cost, ACMRecord *records, uint64_t capacity, uint64_t *n_found, uint64_t sums[2]);
int acm_internal_cpu_replace (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const void *repl_data, const uint64_t *repl_off,
                              uint64_t n_keywords, void *out, uint64_t out_capacity, uint64_t *out_symbols, uint64_t *n_replaced);
int acm_internal_cpu_tokenize (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                               const uint32_t *tok_of, uint64_t n_keywords, uint32_t gap_base, uint32_t mode, uint32_t *tok_id, uint64_t *tok_start,
                               uint32_t *tok_len, uint64_t token_capacity, uint64_t *n_tokens, uint64_t *tok_first, uint64_t *n_selected);
int acm_internal_cpu_grep (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint32_t flags, uint64_t *hits,
                           uint32_t *kept, uint64_t *n_kept, uint64_t *total, void *out, uint64_t out_capacity, uint64_t *out_offsets,
                           uint64_t *out_symbols);
int acm_internal_cpu_tally_batch (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint64_t *row_ptr,
                                  uint32_t *col, uint64_t *val, uint64_t nnz_capacity, uint64_t *nnz, uint64_t *total);
/* acm_rules' host path: acm_internal_cpu_tally_batch into a room of the call's own, then acm_rules_matrix (arguments as acm_rules') */
int acm_internal_cpu_rules (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, const ACMRuleTerm *terms,
                            const uint64_t *rule_ptr, const uint32_t *need, uint64_t n_rules, uint64_t *fired_ptr, uint32_t *fired,
                            uint64_t fired_capacity, uint64_t *n_fired, uint64_t *total);
/* acm_score's host path: the same count matrix, then acm_score_matrix and, when the kept entries had room and k > 0, acm_score_top
 * (arguments as acm_score's) */
int acm_internal_cpu_score (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, const ACMScoreTerm *terms,
                            const uint64_t *class_ptr, const int64_t *bias, const int64_t *threshold, uint64_t n_classes, uint64_t *kept_ptr,
                            uint32_t *kept_class, int64_t *kept_score, uint64_t kept_capacity, uint64_t *n_kept, uint32_t *best, uint32_t k,
                            uint64_t *class_hits, uint32_t *top_n, uint32_t *top_text, int64_t *top_score, uint64_t *total);
/* acm_grep_lines' host path: acm_split_offsets, then acm_internal_cpu_grep (arguments as acm_grep_lines') */
int acm_internal_cpu_grep_lines (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const void *delims, uint32_t n_delims,
                                 uint32_t split_flags, uint32_t grep_flags, uint64_t *n_texts, uint64_t *n_kept, uint64_t *total, void *out,
                                 uint64_t out_capacity, uint64_t *out_symbols, uint64_t texts_capacity, uint64_t *offsets, uint64_t *hits,
                                 uint32_t *kept, uint64_t *out_offsets);
/* WORDS' arguments (include/acm_gpu.h): a symbol size of 1, 2, 4 or 8, 1 .. ACM_WORDS_MAX_RANGES ranges with lo <= hi, flags 1 .. 3 */
int acm_internal_words_args_ok (uint32_t sym_bytes, const void *ranges, uint32_t n_ranges, uint32_t flags);
/* acm_scan_words' host path: the caller loop, then acm_words_records over its records (arguments as acm_scan_words') */
int acm_internal_cpu_scan_words (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const void *ranges, uint32_t n_ranges,
                                 uint32_t flags, ACMRecord *records, uint64_t capacity, uint64_t *n_found);
/* acm_scan_chars' host path: the caller loop, then acm_chars_records over its records (arguments as acm_scan_chars', the symbol size
 * behind n_symbols: anything but 1 is ACM_GPU_E_ARG) */
int acm_internal_cpu_scan_chars (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint32_t unit, ACMRecord *records,
                                 uint64_t *char_start, uint32_t *char_len, uint8_t *edge, uint64_t capacity, uint64_t *n_found);
/* acm_context's host path: the caller loop, then acm_context_records over its records (arguments as acm_context's, the symbol size
 * behind n_symbols; records NULL: a room of the call's own) */
int acm_internal_cpu_context (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records, uint64_t capacity,
                              uint64_t *n_found, uint32_t before, uint32_t after, uint32_t flags, void *out, uint64_t out_capacity,
                              uint64_t *out_symbols, uint64_t *n_snippets, uint64_t *snip_lo, uint64_t *out_offsets, uint32_t *snip_text,
                              uint32_t *rec_snip, int64_t *rec_at);
/* acm_scan_anchored's and acm_lookup's host paths: the caller loop from the root at every offset, then acm_anchored_records over its
 * records (arguments as the public calls'; offsets[] already checked) */
int acm_internal_cpu_scan_anchored (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint32_t mode,
                                    ACMRecord *records, uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found);
int acm_internal_cpu_lookup (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint32_t *whole_id,
                             uint32_t *prefix_id, uint32_t *prefix_len);
/* acm_scan_patterns' checks on every path: acm_patterns_check against the machine's keywords, and every term's length is its keyword's */
int acm_internal_patterns_machine_check (ACMachine *m, const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns);
/* acm_scan_patterns' host path: the caller loop (from the root at every offset when offsets is given), then acm_patterns_records over
 * its records (arguments as acm_scan_patterns', the symbol size behind n_symbols; the public call has checked them) */
int acm_internal_cpu_scan_patterns (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                    const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, ACMRecord *out, uint64_t out_capacity,
                                    uint64_t *n_found);
/* acm_scan_chains' check on every path: acm_chains_check against the machine's keywords */
int acm_internal_chains_machine_check (ACMachine *m, const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains);
/* acm_scan_chains' host path: the caller loop (from the root at every offset when offsets is given), then acm_chains_records over
 * its records (arguments as acm_scan_chains', the symbol size behind n_symbols; the public call has checked them) */
int acm_internal_cpu_scan_chains (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                  const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, ACMRecord *out, uint64_t out_capacity,
                                  uint64_t *n_found);
/* acm_scan_near's check on every path: acm_near_check against the machine's keywords */
int acm_internal_near_machine_check (ACMachine *m, const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups);
/* acm_scan_near's host path: the caller loop (from the root at every offset when offsets is given), then acm_near_records over its
 * records (arguments as acm_scan_near's, the symbol size behind n_symbols; the public call has checked them) */
int acm_internal_cpu_scan_near (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups, ACMRecord *out,
                                uint64_t out_capacity, uint64_t *n_found);
/* acm_scan_approx's checks on every path: acm_approx_check against the machine's keywords, and every term's keyword is spelled as the
 * term's piece of its target, by the machine's comparator over symbols of sym_bytes bytes */
int acm_internal_approx_machine_check (ACMachine *m, uint32_t sym_bytes, const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                                       const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets);
/* acm_scan_approx's host path: the caller loop (from the root at every offset when offsets is given), then the sequential APPROX over
 * its records with symbols compared by the machine's comparator (arguments as acm_scan_approx', the symbol size behind n_symbols; the
 * public call has checked them) */
int acm_internal_cpu_scan_approx (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                  const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms,
                                  const uint64_t *tgt_ptr, uint64_t n_targets, ACMRecord *out, uint32_t *dist, uint64_t out_capacity,
                                  uint64_t *n_found);
/* acm_scan_edit's checks on every path: acm_internal_approx_machine_check plus the edit calls' two conditions (k[w] <= 15, k[w] < L_w) */
int acm_internal_edit_machine_check (ACMachine *m, uint32_t sym_bytes, const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                                     const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets);
/* acm_scan_edit's host path: acm_internal_cpu_scan_approx with the sequential EDIT behind the caller loop */
int acm_internal_cpu_scan_edit (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms,
                                const uint64_t *tgt_ptr, uint64_t n_targets, ACMRecord *out, uint32_t *dist, uint64_t out_capacity,
                                uint64_t *n_found);
/* acm_scan_templates' checks on every path: acm_templates_check against the machine's keywords plus acm_scan_approx's on the terms */
int acm_internal_templates_machine_check (ACMachine *m, uint32_t sym_bytes, const ACMTemplateSpec *spec);
/* acm_scan_templates' host path: acm_internal_cpu_scan_approx with the cells (literal cells by the comparator, class cells by value) */
int acm_internal_cpu_scan_templates (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                     const ACMTemplateSpec *spec, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found);
void acm_internal_set_scan_path (ACMachine *m, int path);
/* ACM_NMEYER_85 builds: brings failure links and output counts up to date (no-op otherwise);
 * takes the machine lock itself */
void acm_internal_refresh (ACMachine *m);
void acm_internal_lock (ACMachine *m);
void acm_internal_unlock (ACMachine *m);
/* acm_get_keyword for callers that already hold the machine lock */
int acm_internal_get_keyword (const ACMachine *m, uint32_t keyword_id, MatchHolder *matcher);
/* serialises the users of the machine's cached device plan (acm_scan) */
void acm_internal_plan_lock (ACMachine *m);
void acm_internal_plan_unlock (ACMachine *m);
/* per-machine slot for the cached device plan (owned by acm_gpu.hip) */
void **acm_internal_plan_slot (ACMachine *m);
/* set by the device side once; called by acm_release to drop the cached plan */
extern void (*acm_internal_plan_dropper) (void *plan);

#ifdef __cplusplus
}
#endif
#endif
