/*
 * acm_segment.h -- the minimum-cost tiling of a text by keywords: SEGMENT of a record set.
 * Part of include/acm_gpu.h, which includes this file at its end; everything there applies
 * (ACMRecord, the error codes, `d_` pointers, `stream` arguments).
 *
 * SELECT (acm_gpu.h) is the greedy tiling: leftmost first, longest at a tie -- MaxMatch.  A unigram
 * tokeniser, a word segmenter, a replacer whose entries carry priorities and a compound splitter
 * want another one: every keyword has a cost, every symbol no chosen keyword covers has a cost, and
 * the tiling of the smallest total is taken.  On `abcd` with {ab, abc, cd} SELECT takes `abc` and
 * strands `d`; every sensible cost table wants `ab` + `cd`.  The output is a selection exactly as
 * SELECT's, so acm_gpu_tokens_records_device, acm_gpu_replace_records_device,
 * acm_gpu_context_records_device and acm_gpu_words_records_device take it as they are.
 *
 * DEFINITION.  Inputs: a record set R in canonical order (end_pos ascending, length descending at
 * an equal end; a record's start is end_pos + 1 - length); cost[0 .. n_keywords), every value below
 * 2^24; gap_cost below 2^24 (the limits keep every sum below 2^64 over any span the order passes
 * take, 2^40 positions; zero is allowed for both).  A TILING is a subset of R in which no two
 * records share a symbol; its cost over a range of n symbols is the sum of cost[keyword_id] over its
 * records plus gap_cost times the number of symbols it leaves uncovered.  SEGMENT (R) is the tiling
 * the following rule fixes, positions taken relative to any pos_lo at or below every start, n
 * reaching at least past every end:
 *     1. best[0] = 0;
 *     2. for p = 1 .. n: best[p] = the smaller of best[p - 1] + gap_cost and the minimum of
 *        best[start_r] + cost[kw_r] over the records r with end_r = p - 1;
 *     3. backwards from p = n: let M be the records with end_r = p - 1 and best[start_r] + cost[kw_r]
 *        == best[p].  If M is not empty, emit its longest record (the smaller keyword_id at an equal
 *        length) and set p = start_r; otherwise p = p - 1.  Stop at p = 0.
 * So a keyword wins a tie against uncovered symbols, a longer last piece wins a tie against a
 * shorter one, and ties are resolved from the right.  The result is a tiling of minimum cost and
 * does not depend on pos_lo or n.  The output is in canonical order and is a selection in exactly
 * REPLACE's and TOKENS' sense.  A batch's records never cross a text boundary, so SEGMENT of a
 * batch's records is the concatenation of SEGMENT of every text's.
 *
 *     text        keywords and costs           gap   SEGMENT                                   cost
 *     ushers      he, she, his, hers: 1 each     2   (end 5, length 4, hers)                      5
 *     abcd        ab, abc, cd: 1 each           10   (1, 2, ab), (3, 2, cd)                       2
 *     a x 1001    a = 2, aa = 4                  2   (0, 1, a), then 500 x aa at starts 1, 3, ..  2002
 *     a x 1000    a = 5, aa = 6, aaa = 100       7   500 x aa                                  3000
 * (SELECT gives (2, 3, abc) on the second row and puts the single `a` of the third at the end.)
 *
 * sums (may be NULL): sums[0] = the sum of cost[keyword_id] over the emitted records, sums[1] = the
 * sum of their lengths; the tiling's cost over the caller's own range is sums[0] + gap_cost *
 * (n_symbols - sums[1]).
 *
 * acm_segment_records: SEGMENT of records[0 .. n) in place in the front of the array, as
 * acm_select_records works; the plain sequential pass on the host, no device.  Positions are taken
 * relative to the first record's end, so any 64-bit end_pos is taken (bit 63 included) and a start
 * may lie in front of position 0.  ACM_GPU_E_ARG, with nothing modified: a NULL argument that is needed, a cost or
 * gap_cost of 2^24 or more, a keyword_id >= n_keywords, a length of 0, an end_pos that decreases, a
 * span of 2^40 positions or more.
 *
 * acm_gpu_segment_records_device: the same on the device (dev_segment.h).  Everything not said here
 * is acm_gpu_select_records_device's, word for word: d_n and n_or_capacity (below 2^31), the range
 * [pos_lo, pos_lo + span), the plan's lmax, the overflow rule (*d_n > n_or_capacity: nothing is
 * selected, *d_count = *d_n, d_sums is zero), d_out may be d_records and d_count may be d_n, a record
 * that breaks SELECT's contract is dropped with the plan's error flag raised.  The call only queues
 * launches on `stream`: there is no host round trip for any record set (the records stay in canonical
 * order, no order pass runs), and no launch geometry depends on a count that lives on the device.
 * d_cost (device) holds n_keywords costs.  A keyword_id >= n_keywords or a cost of 2^24 or more in
 * d_cost is seen by a validation pass before any address or sum is formed from it: *d_count = 0,
 * nothing else is written and acm_gpu_plan_status reports ACM_GPU_E_INTERNAL.  gap_cost of 2^24 or
 * more is ACM_GPU_E_ARG.  d_sums (device, 16 bytes, may be NULL) receives sums[].  Records that are
 * not in canonical order give an unspecified result; nothing is read or written out of bounds.
 * d_tmp must hold acm_gpu_segment_tmp_bytes (plan, n_or_capacity, span) bytes (about 50 bytes per
 * record of capacity).  Two knobs in the environment, read at every call (and by the *_tmp_bytes
 * functions), let tests cross every seam at small sizes: ACM_GPU_SEGMENT_LONG=<records>, the size
 * from which a group of records chained by shared symbols is taken by a whole wave instead of a
 * lane, and ACM_GPU_SEGMENT_TILE=<records>, a multiple of 64, the tile of the group and compaction
 * passes.
 *
 * acm_gpu_scan_segment_device: acm_gpu_scan_tokens_device's pattern.  With d_offsets == NULL
 * acm_gpu_scan_ordered_device with emit_from = 0, with offsets (pos_base must be 0 then)
 * acm_gpu_scan_batch_device, then the pass above over [pos_base, pos_base + n_symbols), all on
 * `stream`.  CAPACITY is select's rule: all matches must fit, and *d_count > capacity names a
 * capacity that suffices (the records are unspecified then, d_sums is zero).  n_keywords below
 * acm_gpu_tally_keywords (plan) is ACM_GPU_E_ARG.  d_tmp must hold acm_gpu_scan_segment_tmp_bytes
 * (plan, capacity, n_symbols, n_texts) bytes.
 * acm_gpu_scan_segment_host: the same from host memory, blocking; on ACM_GPU_E_OVERFLOW *n_found
 * holds a capacity that suffices.  A cost of 2^24 or more is ACM_GPU_E_ARG.
 * acm_segment: the call on the machine itself, total over machines exactly as acm_select is (same
 * three paths, same cached plan and acm_gpu_plan_update, acm_scan_path says which ran): the GPU paths
 * run acm_gpu_scan_segment_host, ACM_SCAN_PATH_CPU_LOOP runs the caller loop on the host and then
 * acm_segment_records.  A missing device stays an error, never a fallback.
 * Out of scope: sums per text, several GPUs (segment on one device), flows.
 */
#ifndef ACM_SEGMENT_H_AMD
#define ACM_SEGMENT_H_AMD

#include "acm_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

int acm_segment_records (ACMRecord *records, uint64_t n, const uint32_t *cost, uint64_t n_keywords,
                         uint32_t gap_cost, uint64_t *n_selected, uint64_t sums[2] /* may be NULL */);
size_t acm_gpu_segment_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t span);
int acm_gpu_segment_records_device (ACMPlan *plan, const ACMRecord *d_records, uint64_t n_or_capacity,
                                    const uint64_t *d_n /* device count, may be NULL: n is the count */,
                                    uint64_t pos_lo, uint64_t span,
                                    const uint32_t *d_cost, uint64_t n_keywords, uint32_t gap_cost,
                                    ACMRecord *d_out, uint64_t *d_count, uint64_t *d_sums /* 16 bytes, may be NULL */,
                                    void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_segment_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_segment_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                 const uint64_t *d_offsets /* NULL: one text */, uint64_t n_texts,
                                 const uint32_t *d_cost, uint64_t n_keywords, uint32_t gap_cost,
                                 ACMRecord *d_records, uint64_t capacity, uint64_t *d_count, uint64_t *d_sums,
                                 void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_segment_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                               const uint64_t *offsets, uint64_t n_texts,
                               const uint32_t *cost, uint64_t n_keywords, uint32_t gap_cost,
                               ACMRecord *records, uint64_t capacity, uint64_t *n_found, uint64_t sums[2]);   /* blocking */
int acm_segment (ACMachine *machine, const void *text, uint64_t n_symbols,
                 const uint32_t *cost, uint64_t n_keywords, uint32_t gap_cost,
                 ACMRecord *records, uint64_t capacity, uint64_t *n_found, uint64_t sums[2]);

#ifdef __cplusplus
}
#endif
#endif
