/*
 * acm_near.h -- unordered keyword proximity: NEAR/n groups, NEAR of a record set.
 * Part of include/acm_gpu.h, which includes this file at its end; everything there applies (the
 * error codes, `d_` pointers, `stream` arguments, the batch and the offsets contract).
 *
 * CHAINS joins keyword records in a fixed order with bounded gaps.  Proximity search leaves the order
 * open: `error NEAR/40 disk`, "any three of these five indicator terms within 200 symbols of one
 * line", `ssn` within 30 symbols of `social security` in either order.  As chains a NEAR of m terms
 * needs m! of them, and a chain forbids overlapping terms; acm_rules sees whole texts and knows no
 * distance.  NEAR is that join.  It is a pure function of a record set in canonical order, exactly as
 * CHAINS is, so it runs behind every plan kind, symbol size, class plan and pending delta alike and has
 * CHAINS' calling shape.
 *
 * DEFINITION.  Terms and groups: a group is a list of m keyword ids (its terms), a `width` and a
 * `need`.  Group g is terms[group_ptr[g] .. group_ptr[g + 1]), a uint32_t array; group_ptr has n_groups
 * + 1 uint64_t entries; groups[g] is an ACMNearGroup { width, need }.  need == 0 means m.
 * ACM_GPU_E_ARG: a group without terms, more than ACM_NEAR_TERMS_MAX (16) terms, the same keyword id
 * twice in one group, keyword_id >= n_keywords, width == 0 or width > ACM_NEAR_WIDTH_MAX (2^20), need >
 * m, a group_ptr that decreases or does not begin with 0, n_groups >= 2^31, 2^31 terms or more.
 * NEAR (R, offsets, G).  R is a record set in canonical order with positions pos_base + index.  Texts
 * are as in CHAINS: offsets == NULL means one text, empty texts are allowed.  A record's start is s =
 * end + 1 - length.  A COVER of group g that ends at e, with first symbol S, is a set of records of R
 * such that
 *   every record has a keyword of g,
 *   the records have at least `need` distinct keywords between them,
 *   every record lies wholly inside [S, e] (start >= S, end <= e),
 *   at least one record ends at e,
 *   e + 1 - S <= width, and
 *   one text holds S and e.
 * Records of a cover may overlap or nest: `he` inside `she` counts for both.
 * For every pair (g, e) with a cover the output holds exactly one ACMRecord (end_pos = pos_base + e,
 * length = e + 1 - S*, keyword_id = g), S* the greatest S over the covers: the shortest window that
 * ends at e, reported the way CHAINS and acm_scan_edit report.  The output is in the total order
 * end_pos ascending, length descending, group id ascending (CHAINS' order).  A group of one term gives
 * its keyword's records whose length is at most `width`.
 * The definition permits a closed form.  best_u (e) = the greatest start among the records of term u
 * that end at or before e, or none.  A (e) = the terms with a record ending exactly at e, with that
 * record's start a_start.  For a in A (e): S_a = a_start when need == 1, else the smaller of a_start
 * and the (need - 1)-th greatest best_u over u != a, none if fewer than need - 1 such terms exist.
 * S* = the greatest S_a, kept if S* >= max (the begin of e's text, e + 1 - width).
 *
 * acm_near_check: the argument checks above, no device; every other entry point runs it.
 * acm_near_records: the plain sequential NEAR on the host, no device, acm_chains_records' contract:
 * ACM_GPU_E_OVERFLOW with *n_found = the entries needed when out_capacity is too small (`out` is
 * untouched then), out == NULL with capacity 0 only counts, ACM_GPU_E_ARG with nothing written for
 * offsets that break the batch contract and for a record outside [pos_base, pos_base + n_symbols) (its
 * end or its start) or of length 0.
 *
 * acm_gpu_near_create compiles a set once on the host and uploads it to the plan's device (ACMNear,
 * opaque like ACMChains): an index inverted by keyword.  A keyword's postings are (group, term index
 * j, width, need, m), by group.  n_keywords is acm_gpu_tally_keywords (plan) at creation; the set stays
 * valid after acm_gpu_plan_update, and a keyword added later nears nothing.
 * acm_gpu_near_info: groups, terms, the most terms of a group, the greatest width and the most
 * postings of one keyword.  n x max_postings bounds the output of n records, so a caller can pick an
 * out_capacity that cannot overflow.
 *
 * acm_gpu_near_records_device (dev_near.h): NEAR of d_records on the device,
 * acm_gpu_chains_records_device's contract: d_n NULL -- n_or_capacity is the number of records; d_n
 * given -- *d_n is, and n_or_capacity the room of d_records.  n_or_capacity, out_capacity and n_texts
 * are below 2^31 (and n_or_capacity x max_postings below 2^40); d_out must not overlap d_records
 * (ACM_GPU_E_ARG).  The call only queues launches on `stream`, with no host round trip; the plan is
 * used for its device, its grid cap and its error word only.  The check of d_offsets in a launch of
 * its own; then ONE walk pass: every record has one slot per posting of its keyword (a fixed stride of
 * max_postings slots), and of the records of a group's keywords that end at e the first in canonical
 * order -- the HEAD of (g, e) -- fills its slot with S* + 1, every other slot is 0.  The head walks the
 * records backwards from the last one that ends at e, keeps the best start per term, and stops as soon
 * as no record further back can change the answer; a walk of more than T records is finished by the
 * whole wave, one such head at a time, 64 records per round.  T is 64 (ACM_GPU_NEAR_COOP=<records> in
 * the environment sets another, read at every call: 0 makes every walk cooperative, a huge value none;
 * both forms give the same output).  Then a count pass over the slots, a 64-bit exclusive sum, a fill
 * pass and PATTERNS' order pass over every group of equal end_pos.  Tiles of 256 records
 * (ACM_GPU_NEAR_TILE=<records>: a multiple of 64 from 64 to 1 Mi, read at every call).  Both defaults
 * are measured on one workload only (tools/exp_near.py): T is CHAINS' own and within 15 %
 * of the better of 0 and "none" at every width, the tile is the fastest of 64, 256, 1,024 and CHAINS'
 * 4,096.  No atomics on global memory decide a result,
 * every slot is written by one lane, and launch geometry and launch count depend on the set and the
 * arguments, never on what the records hold.  d_tmp must hold acm_gpu_near_tmp_bytes (plan, near,
 * n_or_capacity, n_texts) bytes (0 for a call that would be refused).
 *   *d_count <= out_capacity: the count is exact and d_out is complete and in order.
 *   *d_count > out_capacity: it is the capacity needed, d_out is unspecified, and nothing is written
 *     outside d_out[0 .. out_capacity).
 *   *d_n > n_or_capacity (a scan that overflowed): *d_count = 0 and nothing is written.
 *   d_offsets that break the contract: *d_count = 0, no other output, acm_gpu_plan_status reports
 *     ACM_GPU_E_INTERNAL.
 * A record that breaks the contract (a position outside [pos_base, pos_base + n_symbols), a start
 * below pos_base, a length of 0) is skipped -- it anchors nothing and counts for no term -- and
 * acm_gpu_plan_status reports ACM_GPU_E_INTERNAL (select's rule).  Input that is not in canonical
 * order gives an unspecified result; nothing is read or written out of bounds.
 *
 * acm_gpu_scan_near_device: acm_gpu_scan_ordered_device (emit_from 0) into `capacity` records inside
 * d_tmp, then the passes above; d_tmp must hold acm_gpu_scan_near_tmp_bytes (plan, near, capacity,
 * n_symbols, n_texts) bytes.  *d_found receives the scan's count: when it exceeds `capacity`, *d_count
 * = 0 and *d_found is a capacity that suffices.
 * acm_gpu_scan_near_host: the same from host memory, blocking; it creates and destroys the set itself
 * and sizes the record room from acm_gpu_count_device.  ACM_GPU_E_OVERFLOW means only "out_capacity is
 * too small, *n_found suffices".  Offsets that break the batch contract are ACM_GPU_E_ARG.
 * acm_scan_near: the call on the machine itself, total over machines exactly as acm_scan_chains is
 * (same three paths, same cached plan, same acm_gpu_plan_update; acm_scan_path recorded on success and
 * on overflow).  ACM_SCAN_PATH_CPU_LOOP runs the caller loop per text on the host, then
 * acm_near_records.  A missing device stays an error, never a fallback.
 *
 * Out of scope: terms that are sets of alternative keywords; the same keyword twice in a group ("two
 * occurrences of A"); distances counted in words rather than symbols; all covers rather than one
 * record per end; flows, streams and several GPUs; feeding NEAR records to SELECT or REPLACE (their
 * contract bounds lengths by the plan's lmax).
 */
#ifndef ACM_NEAR_H_AMD
#define ACM_NEAR_H_AMD

#include "acm_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ACM_NEAR_TERMS_MAX 16u
#define ACM_NEAR_WIDTH_MAX (1u << 20)
typedef struct {
  uint32_t width, need;
} ACMNearGroup;
typedef struct ACMNear ACMNear;
typedef struct {
  uint64_t groups, terms, max_terms, max_width, max_postings;
} ACMNearInfo;
int acm_near_check (const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups,
                    uint64_t n_keywords);
int acm_near_records (const ACMRecord *records, uint64_t n, uint64_t n_symbols, uint64_t pos_base,
                      const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                      const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups,
                      uint64_t n_keywords, ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);
int acm_gpu_near_create (ACMPlan *plan, const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups,
                         uint64_t n_groups, ACMNear **out);
void acm_gpu_near_destroy (ACMNear *near);
int acm_gpu_near_info (const ACMNear *near, ACMNearInfo *info);
size_t acm_gpu_near_tmp_bytes (const ACMPlan *plan, const ACMNear *near, uint64_t n_or_capacity, uint64_t n_texts);
int acm_gpu_near_records_device (ACMPlan *plan, const ACMNear *near, const ACMRecord *d_records,
                                 uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                 uint64_t n_symbols, uint64_t pos_base,
                                 const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                 ACMRecord *d_out, uint64_t out_capacity, uint64_t *d_count,
                                 void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_near_tmp_bytes (const ACMPlan *plan, const ACMNear *near, uint64_t capacity,
                                    uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_near_device (ACMPlan *plan, const ACMNear *near, const void *d_text, uint64_t n_symbols,
                              uint64_t pos_base, const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                              uint64_t capacity, ACMRecord *d_out, uint64_t out_capacity,
                              uint64_t *d_count, uint64_t *d_found, void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_near_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                            const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                            const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups,
                            ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);   /* blocking */
int acm_scan_near (ACMachine *machine, const void *text, uint64_t n_symbols,
                   const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                   const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups,
                   ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);

#ifdef __cplusplus
}
#endif
#endif
