/*
 * acm_score.h -- weighted keyword scores per text: SCORE of a count matrix, the best class per text
 * and the best k texts per class.
 * Part of include/acm_gpu.h, which includes this file at its end; everything there applies (the
 * error codes, `d_` pointers, `stream` arguments, the batch and the offsets contract).
 *
 * acm_tally_batch turns a batch of texts into a text x keyword count matrix, acm_rules TESTS that
 * matrix ("A and B", "2 of 5").  A language identifier over n-gram dictionaries, a spam or severity
 * score against a threshold, a topic tagger and a BM25-style ranker WEIGH the keywords instead:
 * every class (a language, a topic, a query) is a weighted sum of capped counts, kept where it
 * reaches a threshold; the best class of a text and the best k texts of a class are wanted on top.
 * These calls do that on the device behind the tally, so that no copy of the matrix goes to the host.
 *
 * DEFINITION.  C[t][k] is acm_tally_batch's matrix; the batch contract, the offsets contract and
 * empty texts are the same as there.
 *   A TERM is ACMScoreTerm { uint32_t keyword_id; int32_t weight; uint32_t cap; }.  Its value for
 *     text t is weight * min (C[t][keyword_id], cap).  cap = ACM_SCORE_NO_CAP (0xFFFFFFFF) is no cap
 *     (a count above 2^32 counts in full), cap = 1 is presence, cap = 0 is ACM_GPU_E_ARG.  weight = 0
 *     is allowed and contributes nothing.
 *   A CLASS c is the terms [class_ptr[c], class_ptr[c + 1]) of terms[] (class_ptr: uint64_t,
 *     n_classes + 1 entries), bias[c] (int64_t) and threshold[c] (int64_t).
 *   The SCORE is S[t][c] = bias[c] + the sum of its terms' values.  A class may have no terms: its
 *     score is its bias everywhere.  A keyword may occur in several terms of one class.
 *   ALL ARITHMETIC IS MODULO 2^64 in two's complement, products included: the result does not depend
 *     on the order of summation, so the device and the host agree bit for bit whatever the atomics
 *     or the sort do.  With counts below 2^31 per (text, keyword) and fewer than 2^31 terms nothing
 *     ever wraps.
 *   ACM_GPU_E_ARG: a class_ptr that decreases or does not begin with 0, a keyword_id >= n_keywords,
 *     cap = 0, n_classes >= 2^31, 2^31 terms or more.
 *   KEPT: the pair (t, c) is kept iff S[t][c] >= threshold[c], compared as signed numbers.  The
 *     RESULT is the kept part of S in CSR form: kept_ptr[0 .. n_texts] (uint64_t, kept_ptr[0] = 0),
 *     row t is kept_class[] (uint32_t, strictly ascending) and kept_score[] (int64_t) at
 *     [kept_ptr[t], kept_ptr[t + 1]); n_kept = kept_ptr[n_texts].
 *   ALWAYS-CLASSES: a class with bias[c] >= threshold[c] is kept on a text with no keyword at all,
 *     an empty text among them; threshold = INT64_MIN keeps every text.  They are the always-rules of
 *     acm_rules over again.
 *   BEST (may be NULL): best[t] (uint32_t) is the class of the largest kept score of row t, at a tie
 *     the smaller class id; ACM_SCORE_NONE (0xFFFFFFFF) for an empty row.  It is written together
 *     with the kept entries: a call that only counts, or whose room is too small, leaves it alone.
 *   TOP (k from 0 to ACM_SCORE_TOP_MAX = 256).  For every class c the kept pairs of column c are
 *     ordered by score descending, at a tie by text id ascending.  class_hits[c] (uint64_t) is the
 *     number of kept texts of column c, top_n[c] = min (k, class_hits[c]) (uint32_t),
 *     top_text[c * k + j] (uint32_t) and top_score[c * k + j] (int64_t) are the j-th of that order for
 *     j < top_n[c] and ACM_SCORE_NONE and 0 beyond.  The order is total, so the result depends on
 *     nothing but S.  k = 0 in a call that also evaluates means none of this; acm_score_top and
 *     acm_gpu_score_top_device with k = 0 give class_hits and top_n = 0 alone.
 *   Outputs are SET, not added to.
 * Keyword ids are first-insertion ranks: a model stays valid when the dictionary grows
 * (acm_gpu_plan_update); keywords added later occur in no term.
 *
 * EXAMPLE (the boundary model of the tests).  Keywords he, she, hers, s, qux = ids 0 .. 4; 14 texts:
 * "", "us", "hers and sh", "e sells she", "", "on top", "", "hers", "xhe", "rs", "s",
 * "ushers he she hers", "", "".  Text 11 holds he 4, she 2, hers 2, s 4.
 *   class  bias  threshold  terms (keyword, weight, cap)        what it shows
 *     0      0       1      (he, 3, -), (hers, 5, -)            a plain sum: text 11 scores 22, "hers" 8, "xhe" 3; kept in 5 texts
 *     1      0       3      (s, 2, 2)                           saturation: "e sells she" has three s and scores 4, not 6;
 *                                                                kept in texts 2, 3, 11, all at 4: a three-way tie for TOP
 *     2      2       1      (he, -4, -), (s, 1, -)              an always-class that he switches off: "hers" scores -1, text 11
 *                                                                -10; texts 1, 9, 10 score 3; empty texts 2; kept in 10 texts
 *     3      0       1      (she, 1, 1), (she, 10, -)           one keyword twice: text 3 scores 11, text 11 scores 21;
 *                                                                a column of 2 kept texts
 *     4      0       1      (qux, 7, -)                         a keyword no text holds: an empty column, top_n = 0
 *     5      0       0      (he, 1, -), (she, -1, -)            cancelling: text 3 is touched and sums to 0; an always-class at
 *                                                                threshold 0, kept in all 14 texts
 *     6     -5      -5      (hers, -2^31, -), (s, 2^31 - 1, 1)  the extreme weights: text 1 scores 2147483642, text 11
 *                                                                -2147483654; kept in 11 texts
 *     7      0       7      (he, 3, -), (s, 1, 3)               kept in text 11 alone (15); "hers and sh" reaches 5,
 *                                                                "e sells she" 6
 * Rows have 2 to 6 kept classes, there are 46 kept pairs, and best of the empty texts is class 2
 * (score 2 beats 0 and -5).
 *
 * acm_score_check: the argument checks above, no device; every other entry point runs it.
 * acm_score_matrix: the plain sequential evaluation of a given count matrix (row_ptr, col, val as
 * acm_tally_batch gives them) on the host, in unsigned arithmetic.  ACM_GPU_E_OVERFLOW with *n_kept =
 * the entries needed when kept_capacity is too small: kept_class, kept_score and best are untouched
 * then, kept_ptr is written all the same.  kept_class or kept_score NULL: the call only counts and
 * returns ACM_GPU_OK.  A row_ptr that decreases or does not begin with 0 and a col >= n_keywords are
 * ACM_GPU_E_ARG (acm_rules_matrix's rule).
 * acm_score_top: TOP of a kept matrix on the host.  ACM_GPU_E_ARG: k > ACM_SCORE_TOP_MAX, a kept_ptr
 * that decreases or does not begin with 0, a kept_class >= n_classes, n_texts or n_classes >= 2^31.
 * top_text and top_score may be NULL when k = 0.
 *
 * acm_gpu_score_create: a model is compiled once, on the host, into an index inverted by keyword
 * and uploaded to the plan's device: post_ptr[n_keywords + 1], the postings (class, weight, cap) of
 * every keyword (a term of weight 0 has none), bias[], threshold[] and the ascending list of the
 * always-classes.  n_keywords is acm_gpu_tally_keywords (plan) at creation; the model belongs to the
 * plan's device and serves that plan, also after acm_gpu_plan_update.  acm_gpu_score_info waits for
 * the device and reports classes, terms, postings, always-classes and how many texts the model's
 * evaluations have sent through the fast and through the wide form since creation (below).
 *
 * acm_gpu_score_matrix_device: the evaluation of ANY count matrix that lies on the device,
 * acm_gpu_tally_batch_device's or a caller's own (rows ascending by keyword id without repeats).
 * The contract is acm_gpu_rules_matrix_device's, word for word, where nothing else is said here.  One
 * wave takes one text (dev_score.h): every posting of every keyword of the row is an item (class,
 * value); the items are sorted by class in the wave's LDS and summed per class; class c is kept iff
 * bias[c] + sum >= threshold[c]; the sorted touched classes are merged with the always-list (a
 * touched always-class may drop out).  A text with more items than the fast form has room for is
 * taken by a block that sorts in scratch (the wide form: slower, always correct).  A count pass fills
 * d_kept_ptr, a fill pass d_kept_class, d_kept_score and d_best.  Outputs, all device memory, valid
 * when `stream` has passed:
 *     *d_n_kept <= kept_capacity:  every output is complete.
 *     *d_n_kept > kept_capacity:  it is the capacity needed; d_kept_ptr is complete and valid, the
 *         rest unspecified; nothing is written outside d_kept_class / d_kept_score[0 .. kept_capacity)
 *         and d_best[0 .. n_texts).
 * d_kept_class and d_kept_score may both be NULL with kept_capacity = 0: the call only counts (and
 * leaves d_best alone).  d_best may be NULL.  A d_row_ptr that breaks the contract: *d_n_kept = 0,
 * nothing else is written, acm_gpu_plan_status reports ACM_GPU_E_INTERNAL, and no address is formed
 * from a row pointer before the check has seen it.  A d_col entry >= the model's n_keywords is
 * skipped, not flagged.  n_texts >= 2^31 is ACM_GPU_E_ARG; n_texts = 0 gives kept_ptr[0] = 0 and
 * n_kept = 0.  d_tmp must hold acm_gpu_score_matrix_tmp_bytes (plan, score, n_texts) bytes.  In the
 * environment, read at every call (tests, experiments): ACM_GPU_SCORE_ITEMS=<1 to 4,096> is the
 * widest text, in items, that takes the fast form (1,024 when absent).  The call only queues
 * launches on `stream`, with no host round trip.
 * acm_gpu_score_top_device: TOP of ANY kept matrix that lies on the device (dev_score.h: a histogram
 * of d_kept_class, its exclusive sum, a scatter of 128-bit keys by class, one block per class that
 * keeps the running best k).  kept_capacity is the room of d_kept_class and d_kept_score.  A
 * d_kept_class >= n_classes is not counted and raises the plan's error flag.  A d_kept_ptr that
 * decreases or does not begin with 0 raises the flag and nothing is written.  d_kept_ptr[n_texts] >
 * kept_capacity (the overflow above): nothing is read from the kept entries, d_class_hits and d_top_n
 * are zero.  k > ACM_SCORE_TOP_MAX, n_texts or n_classes >= 2^31 are ACM_GPU_E_ARG.  d_tmp must hold
 * acm_gpu_score_top_tmp_bytes (plan, kept_capacity, n_classes) bytes: 16 per entry of the room and
 * 24 per class.  Only queues launches; no launch geometry depends on a count on the device.  In the
 * environment, read at every call (tests): ACM_GPU_SCORE_TOP_BLOCKS=<1 to 65,536> is the most blocks of
 * the last pass, which takes a class per block and strides.
 * acm_gpu_score_device: acm_gpu_tally_batch_device into a matrix inside d_tmp, then the evaluation,
 * then -- when k > 0 and d_class_hits, d_top_n, d_top_text and d_top_score are given -- TOP, queued in
 * one call.  Windows, `capacity`, pair_capacity, *d_total, *d_need and *d_need_pairs are exactly
 * tally_batch's; when a window or the pairs overflowed, or d_offsets break the contract, *d_n_kept = 0
 * and nothing else is written.  When *d_n_kept > kept_capacity the top pass does not run: d_top_n[]
 * and d_class_hits[] are zero.  d_tmp must hold acm_gpu_score_tmp_bytes (plan, score, window_symbols,
 * capacity, pair_capacity, n_symbols, n_texts, kept_capacity, k) bytes.
 * acm_gpu_score_host: the same from host memory, blocking, with the model arrays: it creates and
 * destroys the model itself and picks and repeats the rooms exactly as acm_gpu_rules_host does.
 * ACM_GPU_E_OVERFLOW means only "kept_capacity is too small, *n_kept suffices": kept_ptr, total and
 * n_kept are valid then, every other output untouched.  kept_class or kept_score NULL: the call only
 * counts (no best, no top).
 * acm_score: the call on the machine itself, total over machines exactly as acm_rules is (same three
 * paths, same cached plan, acm_scan_path recorded on success and on an output overflow): the GPU
 * paths run acm_gpu_score_host, ACM_SCAN_PATH_CPU_LOOP runs acm_tally_batch's host loop, then
 * acm_score_matrix and acm_score_top.  A missing device stays an error, never a fallback.
 * Out of scope: float weights and length normalisation (the caller's: INTEGRATION.md), a top-k
 * carried across calls, k above 256, TOP without room for the kept matrix, positional weights,
 * flows, several GPUs.
 */
#ifndef ACM_SCORE_H_AMD
#define ACM_SCORE_H_AMD

#include "acm_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ACM_SCORE_NO_CAP 0xFFFFFFFFu
#define ACM_SCORE_NONE 0xFFFFFFFFu
#define ACM_SCORE_TOP_MAX 256u
typedef struct {
  uint32_t keyword_id;
  int32_t weight;
  uint32_t cap;
} ACMScoreTerm;
typedef struct ACMScore ACMScore;
typedef struct {
  uint64_t classes, terms, postings, always_classes;
  uint64_t fast_texts, wide_texts; /* texts evaluated by either form since creation (count passes) */
} ACMScoreInfo;

int acm_score_check (const ACMScoreTerm *terms, const uint64_t *class_ptr, const int64_t *bias,
                     const int64_t *threshold, uint64_t n_classes, uint64_t n_keywords);
int acm_score_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts,
                      uint64_t n_keywords, const ACMScoreTerm *terms, const uint64_t *class_ptr,
                      const int64_t *bias, const int64_t *threshold, uint64_t n_classes,
                      uint64_t *kept_ptr /* n_texts + 1 */, uint32_t *kept_class, int64_t *kept_score,
                      uint64_t kept_capacity, uint64_t *n_kept, uint32_t *best /* n_texts, may be NULL */);
int acm_score_top (const uint64_t *kept_ptr, const uint32_t *kept_class, const int64_t *kept_score,
                   uint64_t n_texts, uint64_t n_classes, uint32_t k, uint64_t *class_hits /* n_classes */,
                   uint32_t *top_n /* n_classes */, uint32_t *top_text /* n_classes * k */,
                   int64_t *top_score /* n_classes * k */);
int acm_gpu_score_create (ACMPlan *plan, const ACMScoreTerm *terms, const uint64_t *class_ptr,
                          const int64_t *bias, const int64_t *threshold, uint64_t n_classes, ACMScore **out);
void acm_gpu_score_destroy (ACMScore *score);
int acm_gpu_score_info (const ACMScore *score, ACMScoreInfo *info);
size_t acm_gpu_score_matrix_tmp_bytes (const ACMPlan *plan, const ACMScore *score, uint64_t n_texts);
int acm_gpu_score_matrix_device (ACMPlan *plan, const ACMScore *score, const uint64_t *d_row_ptr,
                                 const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts,
                                 uint64_t *d_kept_ptr /* n_texts + 1 */, uint32_t *d_kept_class,
                                 int64_t *d_kept_score, uint64_t kept_capacity, uint64_t *d_n_kept,
                                 uint32_t *d_best /* n_texts, may be NULL */, void *d_tmp, size_t tmp_bytes,
                                 void *stream);
size_t acm_gpu_score_top_tmp_bytes (const ACMPlan *plan, uint64_t kept_capacity, uint64_t n_classes);
int acm_gpu_score_top_device (ACMPlan *plan, const uint64_t *d_kept_ptr, const uint32_t *d_kept_class,
                              const int64_t *d_kept_score, uint64_t kept_capacity, uint64_t n_texts,
                              uint64_t n_classes, uint32_t k, uint64_t *d_class_hits, uint32_t *d_top_n,
                              uint32_t *d_top_text, int64_t *d_top_score, void *d_tmp, size_t tmp_bytes,
                              void *stream);
size_t acm_gpu_score_tmp_bytes (const ACMPlan *plan, const ACMScore *score, uint64_t window_symbols,
                                uint64_t capacity, uint64_t pair_capacity, uint64_t n_symbols,
                                uint64_t n_texts, uint64_t kept_capacity, uint32_t k);
int acm_gpu_score_device (ACMPlan *plan, const ACMScore *score, const void *d_text, uint64_t n_symbols,
                          const uint64_t *d_offsets, uint64_t n_texts, uint64_t window_symbols,
                          uint64_t capacity, uint64_t pair_capacity, uint64_t *d_kept_ptr /* n_texts + 1 */,
                          uint32_t *d_kept_class, int64_t *d_kept_score, uint64_t kept_capacity,
                          uint64_t *d_n_kept, uint32_t *d_best, uint32_t k, uint64_t *d_class_hits,
                          uint32_t *d_top_n, uint32_t *d_top_text, int64_t *d_top_score, uint64_t *d_total,
                          uint64_t *d_need, uint64_t *d_need_pairs, void *d_tmp, size_t tmp_bytes,
                          void *stream);
int acm_gpu_score_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                        const ACMScoreTerm *terms, const uint64_t *class_ptr, const int64_t *bias,
                        const int64_t *threshold, uint64_t n_classes, uint64_t *kept_ptr,
                        uint32_t *kept_class, int64_t *kept_score, uint64_t kept_capacity, uint64_t *n_kept,
                        uint32_t *best, uint32_t k, uint64_t *class_hits, uint32_t *top_n, uint32_t *top_text,
                        int64_t *top_score, uint64_t *total);   /* blocking */
int acm_score (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
               const ACMScoreTerm *terms, const uint64_t *class_ptr, const int64_t *bias,
               const int64_t *threshold, uint64_t n_classes, uint64_t *kept_ptr, uint32_t *kept_class,
               int64_t *kept_score, uint64_t kept_capacity, uint64_t *n_kept, uint32_t *best, uint32_t k,
               uint64_t *class_hits, uint32_t *top_n, uint32_t *top_text, int64_t *top_score,
               uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif
