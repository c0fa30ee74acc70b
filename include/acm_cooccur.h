/*
 * acm_cooccur.h -- the keyword co-occurrence matrix of a batch: which keywords occur together, and in how
 * many texts.  Part of include/acm_gpu.h, which includes this file at its end; everything there applies
 * (the error codes, `d_` pointers, `stream` arguments, the batch and the offsets contract).
 *
 * acm_tally_batch builds the text x keyword count matrix C of a batch; acm_rules and acm_score read it row
 * by row, acm_index column by column, one keyword at a time.  The second-order question -- which keywords
 * occur together -- is the keyword x keyword matrix C^T C and its binary form: the input of PMI, Jaccard,
 * lift and association rules over indicator terms, of the term graph of a log corpus or of
 * an IDS rule set ("which signatures fire together"), and of query expansion over acm_index's postings.
 * These calls build it on the device behind the tally, so that neither a record nor C goes to the host, and
 * sum two such matrices, so that a corpus larger than one call is accumulated batch by batch.
 *
 * DEFINITION.  C[t][k] is acm_tally_batch's matrix; the batch contract, the offsets contract and empty
 * texts are the same as there.  `flags` is a bit set of ACM_COOCCUR_PRODUCT (1) and ACM_COOCCUR_DIAGONAL
 * (2).  `row_limit` (uint64_t): with 0 every text CONTRIBUTES; otherwise a text whose row of C has more
 * than row_limit entries contributes nothing and is counted in `skipped` (pairs grow with the square of a
 * row; a caller caps that here).  For keyword ids a <= b and the contributing texts T:
 *   without PRODUCT  X[a][b] = the number of t in T with C[t][a] > 0 and C[t][b] > 0;
 *   with PRODUCT     X[a][b] = the sum over t in T of C[t][a] * C[t][b].  Products and sums are taken
 *                    MODULO 2^64: plain uint64_t arithmetic, on the host and on the device alike.
 *   Without DIAGONAL only a < b is kept; with it a == b as well: X[a][a] is df[a] (the texts of T that
 *   hold a), or the sum of the squares of a's counts under PRODUCT.
 * The result is the upper triangle of X in CSR form over keywords:
 *   co_ptr[0 .. n_keywords] (uint64_t, co_ptr[0] = 0); row a is the entries [co_ptr[a], co_ptr[a + 1]) of
 *     co_col[] and co_val[].
 *   co_col[] (uint32_t) holds the ids b, STRICTLY ASCENDING within a row, b > a (b >= a with DIAGONAL).
 *   co_val[] (uint64_t) holds X[a][b].  An entry exists exactly where at least one contributing text holds
 *     both keywords, so its value is > 0 unless a PRODUCT sum wrapped.
 *   nnz = co_ptr[n_keywords].
 *   cross is the number of pair INSTANCES: the sum over the contributing texts of r (r - 1) / 2, r the
 *     row's length (r (r + 1) / 2 with DIAGONAL).  It depends on row_ptr, row_limit and DIAGONAL alone;
 *     without PRODUCT the sum of all co_val equals cross.
 *   Outputs are SET, not added to.  The result depends on nothing but C, flags and row_limit.
 * ARGUMENTS.  n_keywords is an argument, as in acm_gpu_tally_device: at least acm_gpu_tally_keywords (plan)
 *   in the calls that scan, and below 2^32; ids at or beyond the plan's have empty rows.  n_texts < 2^31;
 *   a room (cross_capacity, out_capacity) is below 2^31 entries; flags has no other bit.  Anything else is
 *   ACM_GPU_E_ARG.  n_texts = 0 gives an all-zero co_ptr and nnz = cross = skipped = 0.
 * ADD.  Two such matrices A and B over n_keywords_a <= n_keywords_b keywords.  A + B is the entrywise sum
 *   modulo 2^64 over n_keywords_b keywords, on the union of their entries.  The matrix of texts [0, m) plus
 *   the matrix of texts [m, n) under the same flags and row_limit is the matrix of texts [0, n).  Keyword
 *   ids are first-insertion ranks, so a dictionary that grew between the two batches (acm_gpu_plan_update)
 *   is covered: A simply has fewer keywords.
 *
 * EXAMPLE (the boundary batch of acm_index.h).  Keywords he, she, hers, s, qux = ids 0 .. 4; 14 texts:
 * "", "us", "hers and sh", "e sells she", "", "on top", "", "hers", "xhe", "rs", "s",
 * "ushers he she hers", "", "".  By brute-force substring counting, entries as (a,b):value:
 *   flags 0                cross 15, nnz 6,  co_ptr 0,3,5,6,6,6
 *                          (0,1):2 (0,2):3 (0,3):4 (1,2):1 (1,3):2 (2,3):3
 *   DIAGONAL               cross 32, nnz 10, co_ptr 0,4,7,9,10,10
 *                          the above and (0,0):5 (1,1):2 (2,2):3 (3,3):7
 *   PRODUCT                cross 15, nnz 6,  co_ptr 0,3,5,6,6,6
 *                          (0,1):9 (0,2):10 (0,3):22 (1,2):4 (1,3):11 (2,3):11
 *   PRODUCT | DIAGONAL     cross 32, nnz 10, co_ptr 0,4,7,9,10,10
 *                          the above and (0,0):20 (1,1):5 (2,2):6 (3,3):33
 * With row_limit = 3, text 11 (four keywords) is skipped: skipped = 1, and flags 0 gives cross 9, nnz 5,
 * (0,1):1 (0,2):2 (0,3):3 (1,3):1 (2,3):2.  The matrix of texts 0 .. 6 plus that of texts 7 .. 13 is the
 * same under every flags.
 *
 * acm_cooccur_matrix: the plain sequential definition on a given count matrix (row_ptr, col, val as
 * acm_tally_batch gives them: rows ascending by keyword id without repeats) on the host; the reference the
 * device is held against.  It sorts the pair instances: its memory goes by `cross`, never by cross squared
 * or n_keywords squared.  ACM_GPU_E_OVERFLOW with *nnz = the entries needed when out_capacity is too small:
 * co_ptr, *cross and *skipped are written all the same, co_col and co_val are untouched.  co_col or co_val
 * NULL: the call only counts and returns ACM_GPU_OK.  ACM_GPU_E_ARG under acm_index_matrix's rules (a
 * row_ptr that decreases or does not begin with 0, a col >= n_keywords), for a row that does not ascend
 * strictly, plus the limits above; ACM_GPU_E_NOMEM when the pair instances cannot be held.  In the calls
 * that write host memory `cross`, `skipped` and `total` may be NULL.
 * acm_cooccur_add: ADD on the host, a two-pointer merge per row, with the same overflow and count-only
 * rules (out_ptr is written all the same).  ACM_GPU_E_ARG: a pointer array that decreases or does not begin
 * with 0, a col >= n_keywords_b, n_keywords_a > n_keywords_b, n_keywords_b >= 2^32, a room of 2^31 or more.
 * Rows must ascend strictly by col, as every call here writes them.
 *
 * acm_gpu_cooccur_matrix_device: the matrix of ANY count matrix that lies on the device,
 * acm_gpu_tally_batch_device's or a caller's own (rows ascending by keyword id without repeats).  The
 * passes (dev_cooccur.h): a check of d_row_ptr; the pair instances of every text and their exclusive sum;
 * the expansion of every row into its pairs, one lane per slot of the cross room; a radix sort of the
 * packed pairs over the whole room; head flags, their ranks, and (PRODUCT) a running sum of the weights;
 * co_ptr by a bisection per keyword; the fill.  No atomic on global memory decides a result: a value is a
 * run's length, or the difference of the running sums at its two ends, which is exact under wrap.  Outputs,
 * all device memory, valid when `stream` has passed:
 *     *d_cross <= cross_capacity and *d_nnz <= out_capacity:  every output is complete.
 *     *d_cross > cross_capacity:  it is the room needed, known from d_row_ptr alone (exact below 2^32;
 *         beyond, a row's share is taken as 2^32, more than any room); *d_nnz = 0, *d_skipped is valid,
 *         nothing else is written.
 *     *d_nnz > out_capacity:  it is the room needed; d_co_ptr is complete and valid, the rest unspecified;
 *         nothing is written outside d_co_col / d_co_val[0 .. out_capacity).
 * d_co_col and d_co_val may both be NULL with out_capacity = 0: the call only counts (the cross room is
 * still needed).  A d_row_ptr that breaks the contract: *d_nnz = *d_cross = 0, nothing else is written,
 * acm_gpu_plan_status reports ACM_GPU_E_INTERNAL, and no address is formed from a row pointer before the
 * check has seen it.  A d_col entry >= n_keywords: every pair it is a member of is dropped and the same
 * flag is raised; *d_cross counts those pairs all the same.  A row that repeats a keyword or does not
 * ascend is NOT reported on the device (the host function refuses it): its pairs are put into the upper
 * triangle, a repeated keyword gives a diagonal entry even without DIAGONAL.  d_tmp must hold
 * acm_gpu_cooccur_matrix_tmp_bytes (plan, n_texts, n_keywords, cross_capacity) bytes: 16 per text, 40 per
 * slot of the cross room (two keys, two weights, a flag and a rank; the weights stay unused without PRODUCT)
 * plus the radix sort's own scratch, and nothing per keyword.  The call only queues launches on `stream`,
 * with no host round trip; no launch geometry depends on a count on the device.
 * acm_gpu_cooccur_add_device: ADD of two matrices on the device with the same protocol; the cross room
 * needed is nnz (A) + nnz (B), which *d_cross reports.  A check pass sees both pointer arrays; on a
 * violation *d_out_nnz = *d_cross = 0, nothing else is written, and the plan's error flag is raised.  An
 * entry whose col is >= n_keywords_b is dropped and raises the flag.  d_tmp must hold
 * acm_gpu_cooccur_add_tmp_bytes (plan, n_keywords_b, cross_capacity) bytes: 40 per slot and the sort's.
 * acm_gpu_cooccur_device: acm_gpu_tally_batch_device into a matrix inside d_tmp, then the passes above,
 * queued in one call.  Windows, `capacity`, pair_capacity, *d_total, *d_need and *d_need_pairs are exactly
 * tally_batch's; when a window or the pairs overflowed, or d_offsets break the contract, *d_nnz = *d_cross
 * = 0 and nothing else is written.  d_tmp must hold acm_gpu_cooccur_tmp_bytes (plan, window_symbols,
 * capacity, pair_capacity, n_symbols, n_texts, n_keywords, cross_capacity) bytes.
 * Every *_tmp_bytes function returns 0 for arguments its call would refuse.
 * acm_gpu_cooccur_host: the same from host memory, blocking; it picks and repeats the tally's rooms
 * exactly as acm_gpu_index_host does, picks a cross room and repeats once with *d_cross, which is exact.
 * ACM_GPU_E_OVERFLOW means only "out_capacity is too small, *nnz suffices": co_ptr, nnz, cross, skipped and
 * total are valid then.  co_col or co_val NULL: the call only counts.  ACM_GPU_E_NOMEM: 2^31 pair
 * instances or more.
 * acm_cooccur: the call on the machine itself, total over machines exactly as acm_index is (same three
 * paths, same cached plan, acm_scan_path recorded on success and on an output overflow): the GPU paths run
 * acm_gpu_cooccur_host, ACM_SCAN_PATH_CPU_LOOP runs acm_tally_batch's host loop, then acm_cooccur_matrix.
 * n_keywords is at least acm_nb_keywords (machine).  A missing device stays an error, never a fallback.
 * Out of scope: the lower triangle (it is the mirror), pairs across texts or within a distance
 * (acm_scan_near answers by position), triples and longer item sets, normalised measures (PMI, Jaccard and
 * lift are a few lines over X with DIAGONAL: INTEGRATION.md), subtraction of a batch, flows, several GPUs.
 */
#ifndef ACM_COOCCUR_H_AMD
#define ACM_COOCCUR_H_AMD

#include "acm_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ACM_COOCCUR_PRODUCT 1u
#define ACM_COOCCUR_DIAGONAL 2u

int acm_cooccur_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts,
                        uint64_t n_keywords, uint32_t flags, uint64_t row_limit,
                        uint64_t *co_ptr /* n_keywords + 1 */, uint32_t *co_col, uint64_t *co_val,
                        uint64_t out_capacity, uint64_t *nnz, uint64_t *cross, uint64_t *skipped);
int acm_cooccur_add (const uint64_t *a_ptr, const uint32_t *a_col, const uint64_t *a_val, uint64_t n_keywords_a,
                     const uint64_t *b_ptr, const uint32_t *b_col, const uint64_t *b_val, uint64_t n_keywords_b,
                     uint64_t *out_ptr /* n_keywords_b + 1 */, uint32_t *out_col, uint64_t *out_val,
                     uint64_t out_capacity, uint64_t *out_nnz);
size_t acm_gpu_cooccur_matrix_tmp_bytes (const ACMPlan *plan, uint64_t n_texts, uint64_t n_keywords,
                                         uint64_t cross_capacity);
int acm_gpu_cooccur_matrix_device (ACMPlan *plan, const uint64_t *d_row_ptr, const uint32_t *d_col,
                                   const uint64_t *d_val, uint64_t n_texts, uint64_t n_keywords, uint32_t flags,
                                   uint64_t row_limit, uint64_t cross_capacity,
                                   uint64_t *d_co_ptr /* n_keywords + 1 */, uint32_t *d_co_col, uint64_t *d_co_val,
                                   uint64_t out_capacity, uint64_t *d_nnz, uint64_t *d_cross, uint64_t *d_skipped,
                                   void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_cooccur_add_tmp_bytes (const ACMPlan *plan, uint64_t n_keywords_b, uint64_t cross_capacity);
int acm_gpu_cooccur_add_device (ACMPlan *plan, const uint64_t *d_a_ptr, const uint32_t *d_a_col,
                                const uint64_t *d_a_val, uint64_t n_keywords_a, const uint64_t *d_b_ptr,
                                const uint32_t *d_b_col, const uint64_t *d_b_val, uint64_t n_keywords_b,
                                uint64_t cross_capacity, uint64_t *d_out_ptr /* n_keywords_b + 1 */,
                                uint32_t *d_out_col, uint64_t *d_out_val, uint64_t out_capacity,
                                uint64_t *d_out_nnz, uint64_t *d_cross, void *d_tmp, size_t tmp_bytes,
                                void *stream);
size_t acm_gpu_cooccur_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity,
                                  uint64_t pair_capacity, uint64_t n_symbols, uint64_t n_texts,
                                  uint64_t n_keywords, uint64_t cross_capacity);
int acm_gpu_cooccur_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets,
                            uint64_t n_texts, uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity,
                            uint64_t n_keywords, uint32_t flags, uint64_t row_limit, uint64_t cross_capacity,
                            uint64_t *d_co_ptr /* n_keywords + 1 */, uint32_t *d_co_col, uint64_t *d_co_val,
                            uint64_t out_capacity, uint64_t *d_nnz, uint64_t *d_cross, uint64_t *d_skipped,
                            uint64_t *d_total, uint64_t *d_need, uint64_t *d_need_pairs, void *d_tmp,
                            size_t tmp_bytes, void *stream);
int acm_gpu_cooccur_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                          uint64_t n_keywords, uint32_t flags, uint64_t row_limit,
                          uint64_t *co_ptr /* n_keywords + 1 */, uint32_t *co_col, uint64_t *co_val,
                          uint64_t out_capacity, uint64_t *nnz, uint64_t *cross, uint64_t *skipped,
                          uint64_t *total);   /* blocking */
int acm_cooccur (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
                 uint64_t n_keywords, uint32_t flags, uint64_t row_limit, uint64_t *co_ptr /* n_keywords + 1 */,
                 uint32_t *co_col, uint64_t *co_val, uint64_t out_capacity, uint64_t *nnz, uint64_t *cross,
                 uint64_t *skipped, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif
