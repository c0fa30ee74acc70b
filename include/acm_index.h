/*
 * acm_index.h -- the inverted index of a batch: the postings of every keyword, the count matrix transposed.
 * Part of include/acm_gpu.h, which includes this file at its end; everything there applies (the
 * error codes, `d_` pointers, `stream` arguments, the batch and the offsets contract).
 *
 * acm_tally_batch builds the text x keyword count matrix of a batch, acm_rules and acm_score read it
 * row by row.  A search or triage system asks by column first: which texts hold keyword k, and how
 * often?  That is the postings list of k; its length is the document frequency df[k] that an IDF
 * weight is made of (INTEGRATION.md turns df into an acm_score model), and a corpus larger than one
 * call is indexed batch by batch and concatenated per keyword.  These calls transpose the matrix on the
 * device behind the tally, so that no record and no copy of the matrix goes to the host.
 *
 * DEFINITION.  C[t][k] is acm_tally_batch's matrix; the batch contract, the offsets contract and
 * empty texts are the same as there.  The INDEX is C transposed in CSR form over keywords:
 *   post_ptr[0 .. n_keywords] (uint64_t, post_ptr[0] = 0); keyword k's postings are the entries
 *     [post_ptr[k], post_ptr[k + 1]) of post_text[] and post_count[].
 *   post_text[] (uint32_t) is text_base + t, STRICTLY ASCENDING within a keyword.
 *   post_count[] (uint64_t) is C[t][k], always > 0.
 *   nnz = post_ptr[n_keywords]; it equals tally_batch's nnz.  df[k] = post_ptr[k + 1] - post_ptr[k].
 *   total is the sum of all counts: tally_batch's total.
 *   Outputs are SET, not added to.  The result depends on nothing but C and text_base.
 * ARGUMENTS.  n_keywords is an argument, as in acm_gpu_tally_device: at least acm_gpu_tally_keywords
 *   (plan) and below 2^32; ids at or beyond the plan's have empty lists.  text_base + n_texts <= 2^32
 *   and n_texts < 2^31; a room (post_capacity, out_capacity) is below 2^31 entries.  Anything else is
 *   ACM_GPU_E_ARG.  n_texts = 0 gives an all-zero post_ptr and nnz = 0.
 * CONCAT.  Two indexes A and B over n_keywords_a <= n_keywords_b keywords; in every list B's first
 *   text id must be greater than A's last.  Their concatenation is, per keyword, A's list followed by
 *   B's, over n_keywords_b keywords.  The index of texts [0, m) concatenated with the index of texts
 *   [m, n) at text_base = m is the index of texts [0, n).  Keyword ids are first-insertion ranks, so
 *   a dictionary that grew between the two batches (acm_gpu_plan_update) is covered: A simply has
 *   fewer keywords.
 *
 * EXAMPLE (the boundary batch of acm_score.h).  Keywords he, she, hers, s, qux = ids 0 .. 4; 14 texts:
 * "", "us", "hers and sh", "e sells she", "", "on top", "", "hers", "xhe", "rs", "s",
 * "ushers he she hers", "", "".  With text_base = 0, by brute-force substring counting:
 *   keyword  df  postings as text:count
 *     he      5  2:1, 3:1, 7:1, 8:1, 11:4
 *     she     2  3:1, 11:2
 *     hers    3  2:1, 7:1, 11:2
 *     s       7  1:1, 2:2, 3:3, 7:1, 9:1, 10:1, 11:4
 *     qux     0  an empty list
 * post_ptr = 0, 5, 7, 10, 17, 17; nnz = 17; total = 28.  The index of texts 0 .. 6 concatenated with
 * the index of texts 7 .. 13 at text_base = 7 is the same.
 *
 * acm_index_matrix: the plain sequential transposition of a given count matrix (row_ptr, col, val as
 * acm_tally_batch gives them) on the host.  ACM_GPU_E_OVERFLOW with *nnz = the entries needed when
 * post_capacity is too small: post_ptr is written all the same, post_text and post_count are
 * untouched.  post_text or post_count NULL: the call only counts and returns ACM_GPU_OK.
 * ACM_GPU_E_ARG under acm_rules_matrix's rules (a row_ptr that decreases or does not begin with 0, a
 * col >= n_keywords) plus the limits above.
 * acm_index_concat: CONCAT on the host, with the same overflow and count-only rules (out_ptr is
 * written all the same).  ACM_GPU_E_ARG: a pointer array that decreases or does not begin with 0,
 * n_keywords_a > n_keywords_b, n_keywords_b >= 2^32, a list where B's first id is not above A's last.
 *
 * acm_gpu_index_matrix_device: the transposition of ANY count matrix that lies on the device,
 * acm_gpu_tally_batch_device's or a caller's own (rows ascending by keyword id without repeats).  The
 * passes (dev_index.h): a check of d_row_ptr, a count per keyword, its exclusive sum, a scatter of the
 * entries to a cursor per keyword, and every list put in order by text id -- ids are unique within a
 * list, so the result does not depend on how the atomics fell.  A list of up to ACM_GPU_INDEX_LIST
 * entries is sorted in LDS (the FAST form: one wave, or one block for the longer ones); longer lists go
 * through a radix sort of (keyword, text) keys over the room (the WIDE form: slower, always correct,
 * and no slower for one long list than for many).  Outputs, all device memory, valid when `stream`
 * has passed:
 *     *d_nnz <= post_capacity:  every output is complete.
 *     *d_nnz > post_capacity:  it is the room needed; d_post_ptr is complete and valid (df is known
 *         without any room), the rest unspecified; nothing is written outside d_post_text /
 *         d_post_count[0 .. post_capacity).
 * d_post_text and d_post_count may both be NULL with post_capacity = 0: the call only counts.  A
 * d_row_ptr that breaks the contract: *d_nnz = 0, nothing else is written, acm_gpu_plan_status reports
 * ACM_GPU_E_INTERNAL, and no address is formed from a row pointer before the check has seen it.  A
 * d_col entry >= n_keywords is not counted and raises the same flag.  d_forms (may be NULL) receives
 * two uint64_t: the lists put in order by the fast form (1 <= df <= ACM_GPU_INDEX_LIST) and by the
 * wide form in this call, both 0 in a call that fills nothing.  d_tmp must hold
 * acm_gpu_index_matrix_tmp_bytes (plan, n_texts, n_keywords, post_capacity) bytes: 20 per keyword, and
 * 16 more with 32 per entry of the room when n_texts exceeds the longest list of the fast form.  In the
 * environment, read at every call (tests, experiments): ACM_GPU_INDEX_LIST=<1 to 4,096> is the longest
 * list of the fast form (1,024 when absent).  The call only queues launches on `stream`, with no host round trip;
 * no launch geometry depends on a count on the device.
 * acm_gpu_index_concat_device: CONCAT of two indexes on the device, entry-parallel (every output entry
 * finds its keyword by bisection), with the room, overflow and count-only rules above.  A check pass
 * sees the pointer arrays, then every list's boundary (A's last id against B's first); on a violation
 * *d_out_nnz = 0, nothing else is written, and the plan's error flag is raised.  d_tmp must hold
 * acm_gpu_index_concat_tmp_bytes (plan, n_keywords_b) bytes.
 * acm_gpu_index_device: acm_gpu_tally_batch_device into a matrix inside d_tmp, then the transposition,
 * queued in one call.  Windows, `capacity`, pair_capacity, *d_total, *d_need and *d_need_pairs are
 * exactly tally_batch's; when a window or the pairs overflowed, or d_offsets break the contract,
 * *d_nnz = 0 and nothing else is written.  d_tmp must hold acm_gpu_index_tmp_bytes (plan,
 * window_symbols, capacity, pair_capacity, n_symbols, n_texts, n_keywords, post_capacity) bytes.
 * acm_gpu_index_host: the same from host memory, blocking; it picks and repeats the rooms exactly as
 * acm_gpu_rules_host does.  ACM_GPU_E_OVERFLOW means only "post_capacity is too small, *nnz suffices":
 * post_ptr, total and nnz are valid then.  post_text or post_count NULL: the call only counts.
 * acm_index: the call on the machine itself, total over machines exactly as acm_rules is (same three
 * paths, same cached plan, acm_scan_path recorded on success and on an output overflow): the GPU
 * paths run acm_gpu_index_host, ACM_SCAN_PATH_CPU_LOOP runs acm_tally_batch's host loop, then
 * acm_index_matrix.  n_keywords is at least acm_nb_keywords (machine).  A missing device stays an
 * error, never a fallback.
 * Out of scope: positional postings (the positions inside a posting), query evaluation over postings
 * (acm_rules answers per text), compression of the lists, deletion of texts, flows, several GPUs, a
 * collection-frequency output (it is acm_tally's).
 */
#ifndef ACM_INDEX_H_AMD
#define ACM_INDEX_H_AMD

#include "acm_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

int acm_index_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts,
                      uint64_t n_keywords, uint64_t text_base, uint64_t *post_ptr /* n_keywords + 1 */,
                      uint32_t *post_text, uint64_t *post_count, uint64_t post_capacity, uint64_t *nnz);
int acm_index_concat (const uint64_t *a_ptr, const uint32_t *a_text, const uint64_t *a_count,
                      uint64_t n_keywords_a, const uint64_t *b_ptr, const uint32_t *b_text,
                      const uint64_t *b_count, uint64_t n_keywords_b, uint64_t *out_ptr /* n_keywords_b + 1 */,
                      uint32_t *out_text, uint64_t *out_count, uint64_t out_capacity, uint64_t *out_nnz);
size_t acm_gpu_index_matrix_tmp_bytes (const ACMPlan *plan, uint64_t n_texts, uint64_t n_keywords,
                                       uint64_t post_capacity);
int acm_gpu_index_matrix_device (ACMPlan *plan, const uint64_t *d_row_ptr, const uint32_t *d_col,
                                 const uint64_t *d_val, uint64_t n_texts, uint64_t n_keywords,
                                 uint64_t text_base, uint64_t *d_post_ptr /* n_keywords + 1 */,
                                 uint32_t *d_post_text, uint64_t *d_post_count, uint64_t post_capacity,
                                 uint64_t *d_nnz, uint64_t *d_forms /* 2, may be NULL */, void *d_tmp,
                                 size_t tmp_bytes, void *stream);
size_t acm_gpu_index_concat_tmp_bytes (const ACMPlan *plan, uint64_t n_keywords_b);
int acm_gpu_index_concat_device (ACMPlan *plan, const uint64_t *d_a_ptr, const uint32_t *d_a_text,
                                 const uint64_t *d_a_count, uint64_t n_keywords_a, const uint64_t *d_b_ptr,
                                 const uint32_t *d_b_text, const uint64_t *d_b_count, uint64_t n_keywords_b,
                                 uint64_t *d_out_ptr /* n_keywords_b + 1 */, uint32_t *d_out_text,
                                 uint64_t *d_out_count, uint64_t out_capacity, uint64_t *d_out_nnz,
                                 void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_index_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity,
                                uint64_t pair_capacity, uint64_t n_symbols, uint64_t n_texts,
                                uint64_t n_keywords, uint64_t post_capacity);
int acm_gpu_index_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets,
                          uint64_t n_texts, uint64_t window_symbols, uint64_t capacity,
                          uint64_t pair_capacity, uint64_t n_keywords, uint64_t text_base,
                          uint64_t *d_post_ptr /* n_keywords + 1 */, uint32_t *d_post_text,
                          uint64_t *d_post_count, uint64_t post_capacity, uint64_t *d_nnz,
                          uint64_t *d_forms /* 2, may be NULL */, uint64_t *d_total, uint64_t *d_need,
                          uint64_t *d_need_pairs, void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_index_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                        uint64_t text_base, uint64_t *post_ptr /* n_keywords + 1 */, uint64_t n_keywords,
                        uint32_t *post_text, uint64_t *post_count, uint64_t post_capacity, uint64_t *nnz,
                        uint64_t *total);   /* blocking */
int acm_index (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
               uint64_t text_base, uint64_t *post_ptr /* n_keywords + 1 */, uint64_t n_keywords,
               uint32_t *post_text, uint64_t *post_count, uint64_t post_capacity, uint64_t *nnz,
               uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif
