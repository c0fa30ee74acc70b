/*
 * acm_chars.h -- the positions of matches in the caller's own units: UTF-8 character (code point) and UTF-16
 * code unit indices of a byte text.  Part of include/acm_gpu.h, which includes this file at its end;
 * everything there applies (the error codes, `d_` pointers, `stream` arguments, the batch and the offsets
 * contract, the record contract of the passes that take a record set).
 *
 * Every record the engine emits is (end_pos, length, keyword_id) in symbols, and over a byte plan symbols are
 * bytes.  A caller that holds a Python str, a Java or JavaScript string or an editor buffer whose protocol
 * counts UTF-16 units encodes to UTF-8, scans, and needs every match back in the indices of its own string: a
 * byte offset is wrong as a string index as soon as one two-byte character precedes the match.  These calls
 * do that map on the device, beside the records, with one read of the text at memory rate (the RULER) and a
 * lane per record (the MAP), so that no pass over the text runs on the host.
 *
 * DEFINITION.  Structural and total: nothing is validated, every byte string has an answer.
 *   The text is BYTES (sym_bytes == 1): a plan or a machine with another caller symbol size gets
 *   ACM_GPU_E_ARG.  Comparator-class plans over bytes are fine; like WORDS, the passes read the caller's
 *   original bytes, never a class-mapped copy.
 *   Byte b is a CONTINUATION iff (b & 0xC0) == 0x80; it is a WIDE LEAD iff b >= 0xF0.
 *   For 0 <= a <= b <= n_symbols:  starts (a, b) = the number of non-continuation bytes in text[a, b),
 *                                  wides (a, b)  = the number of wide leads in text[a, b).
 *   `unit` is ACM_CHARS_CODEPOINTS (1) or ACM_CHARS_UTF16 (2); anything else is ACM_GPU_E_ARG.
 *   count (a, b) = starts (a, b) under CODEPOINTS, starts (a, b) + wides (a, b) under UTF16.  On valid UTF-8
 *   with a and b on character boundaries CODEPOINTS gives len (text[a:b].decode ()), UTF16 the number of
 *   UTF-16 code units of that slice (a character of four bytes is a surrogate pair).
 *   TEXTS.  offsets[0 .. n_texts] follows the batch contract (first 0, last n_symbols, non-decreasing);
 *   offsets == NULL: the buffer is one text.
 *   POSITIONS.  For a byte position p in [0, n_symbols] let t be the text with offsets[t] <= p <
 *   offsets[t + 1]; for p == n_symbols t is the last text.  out[i] = count (offsets[t], p)  (uint64_t).
 *   RECORDS.  For a record r let s = end_pos + 1 - length - pos_base and e = end_pos - pos_base, t the text of
 *   s, lo = offsets[t], hi = offsets[t + 1].  Then
 *     char_start[r] (uint64_t) = count (lo, s);
 *     char_len[r]   (uint32_t) = count (s, e + 1);
 *     edge[r]       (uint8_t)  = bit 0 (ACM_CHARS_EDGE_START): s is no boundary; bit 1 (ACM_CHARS_EDGE_END):
 *       e + 1 is no boundary.  Position i is a boundary iff i == lo, or i == hi, or i >= n_symbols, or text[i]
 *       is no continuation.  edge == 0 on valid UTF-8 says that the record covers whole characters:
 *       decoded[char_start : char_start + char_len] is the keyword.
 *   A match that spans a cut is mapped like any other (char_len counts through the cut; its end is judged by
 *   the byte behind it).  Nothing is dropped: this is a map, not a filter; output r belongs to input r, and the
 *   input may be in any order.  Each of the three output arrays may be NULL; all three NULL is ACM_GPU_E_ARG.
 *   Outputs are SET, not added to.
 *
 * EXAMPLE (checked against bytes.decode for every record with edge 0).  The text "aé€\U0001F600
 * é\U0001F600a" as UTF-8, 18 bytes: 61 c3 a9 e2 82 ac f0 9f 98 80 20 c3 a9 f0 9f 98 80 61.  Keyword ids
 * 0 .. 5: U+00E9, U+20AC U+1F600, U+1F600, "a", the single byte A9, and the bytes 9F 98 80 20.
 *   (end_pos, length, id)   CODEPOINTS (start, len)   UTF16 (start, len)   edge
 *   ( 0, 1, 3)              (0, 1)                    (0, 1)               0
 *   ( 2, 2, 0)              (1, 1)                    (1, 1)               0
 *   ( 2, 1, 4)              (2, 0)                    (2, 0)               1
 *   ( 9, 7, 1)              (2, 2)                    (2, 3)               0
 *   ( 9, 4, 2)              (3, 1)                    (3, 2)               0
 *   (10, 4, 5)              (4, 1)                    (5, 1)               1
 *   (12, 2, 0)              (5, 1)                    (6, 1)               0
 *   (12, 1, 4)              (6, 0)                    (7, 0)               1
 *   (16, 4, 2)              (6, 1)                    (7, 2)               0
 *   (17, 1, 3)              (7, 1)                    (9, 1)               0
 * The whole text is 8 code points and 10 UTF-16 units.
 *
 * acm_chars_positions, acm_chars_records: the plain sequential definition on the host, no device; the
 * reference the device is held against.  ACM_GPU_E_ARG, with nothing written, for offsets that break the
 * contract, a position above n_symbols, a record outside [pos_base, pos_base + n_symbols), with a start below
 * pos_base, or of length 0; ACM_GPU_E_NOMEM when the prefix counts of the text cannot be held.
 *
 * THE RULER.  acm_gpu_chars_ruler_device builds an opaque rank structure over one text in d_ruler
 * (acm_gpu_chars_ruler_bytes (plan, n_symbols) bytes: at most n_symbols / 16 plus 16 bytes per tile plus a
 * constant; d_tmp: acm_gpu_chars_ruler_tmp_bytes).  It holds both counts, so `unit` is chosen at map time,
 * and it serves any number of record sets over that text: the scan's, the selection's, the whole-word ones,
 * pattern records, token places, snippet bounds.  It belongs to d_text AS IT LIES: the same address and the
 * same n_symbols go to the map calls.  One read of the text, no second pass, no atomic decides a value
 * (dev_chars.h).  ACM_GPU_CHARS_TILE=<bytes> in the environment (a multiple of 256 from 256 to 1 Mi, read
 * at every call) is the tile of the pass; the ruler remembers it.
 * THE MAPS.  acm_gpu_chars_records_device and acm_gpu_chars_positions_device: a lane per record or position.
 * d_n has acm_gpu_words_records_device's meaning: NULL: n_or_capacity is the count; otherwise *d_n is, and
 * *d_n > n_or_capacity means that nothing is written.  A record or position that breaks the contract gets
 * char_start = char_len = 0, edge = ACM_CHARS_EDGE_BAD (4), out = 0, reads nothing out of bounds and raises
 * the plan's error flag: acm_gpu_plan_status reports ACM_GPU_E_INTERNAL.  So does every record under a ruler
 * that was not built over this d_text and n_symbols.  d_offsets that break the contract are found in a launch
 * of their own (no address is formed from an unchecked offset): no output is written, the status is
 * ACM_GPU_E_INTERNAL.  d_tmp must hold acm_gpu_chars_tmp_bytes (plan, n_or_capacity, n_texts) bytes.
 * All these calls only queue launches on `stream`, with no host round trip; no launch geometry depends on
 * device data; they work with any plan kind, a pending delta included, and use the plan for its device, its
 * symbol size and its grid cap only.
 * acm_gpu_scan_chars_device: the ordered scan with emit_from = 0, the ruler (inside d_tmp) and the record map,
 * queued in one call.  `capacity` must hold ALL matches; *d_count > capacity: it is the scan's count and the
 * other outputs are unspecified.  d_tmp: acm_gpu_scan_chars_tmp_bytes (plan, capacity, n_symbols, n_texts).
 * acm_gpu_scan_chars_host: the same from host memory, blocking; ACM_GPU_E_OVERFLOW leaves a capacity that
 * suffices in *n_found.
 * acm_scan_chars: the call on the machine itself, total over machines exactly as acm_scan_words is (same
 * three paths, same cached plan, acm_scan_path recorded on success and on overflow): the GPU paths run
 * acm_gpu_scan_chars_host, ACM_SCAN_PATH_CPU_LOOP runs the caller loop and then acm_chars_records.  A missing
 * device stays an error, never a fallback.
 * Every *_tmp_bytes and *_bytes function returns 0 for arguments its call would refuse.
 * Out of scope: UTF-8 validation, grapheme clusters, the inverse map (character to byte), texts of 2- and
 * 4-byte symbols (surrogates in the text itself), character units inside the other families' signatures,
 * flows, streams of pieces, several GPUs.
 */
#ifndef ACM_CHARS_H_AMD
#define ACM_CHARS_H_AMD

#include "acm_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ACM_CHARS_CODEPOINTS 1u
#define ACM_CHARS_UTF16 2u
#define ACM_CHARS_EDGE_START 1u
#define ACM_CHARS_EDGE_END 2u
#define ACM_CHARS_EDGE_BAD 4u

int acm_chars_positions (const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts,
                         uint32_t unit, const uint64_t *pos, uint64_t n, uint64_t *out);
int acm_chars_records (const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets,
                       uint64_t n_texts, uint32_t unit, const ACMRecord *records, uint64_t n,
                       uint64_t *char_start, uint32_t *char_len, uint8_t *edge);
size_t acm_gpu_chars_ruler_bytes (const ACMPlan *plan, uint64_t n_symbols);
size_t acm_gpu_chars_ruler_tmp_bytes (const ACMPlan *plan, uint64_t n_symbols);
int acm_gpu_chars_ruler_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, void *d_ruler,
                                size_t ruler_bytes, void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_chars_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_texts);
int acm_gpu_chars_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                  const uint64_t *d_offsets, uint64_t n_texts, uint32_t unit, const void *d_ruler,
                                  const ACMRecord *d_records, uint64_t n_or_capacity, const uint64_t *d_n,
                                  uint64_t *d_char_start, uint32_t *d_char_len, uint8_t *d_edge, void *d_tmp,
                                  size_t tmp_bytes, void *stream);
int acm_gpu_chars_positions_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols,
                                    const uint64_t *d_offsets, uint64_t n_texts, uint32_t unit, const void *d_ruler,
                                    const uint64_t *d_pos, uint64_t n, uint64_t *d_out, void *d_tmp,
                                    size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_chars_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_chars_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                               const uint64_t *d_offsets, uint64_t n_texts, uint32_t unit, ACMRecord *d_records,
                               uint64_t *d_char_start, uint32_t *d_char_len, uint8_t *d_edge, uint64_t capacity,
                               uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_chars_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                             const uint64_t *offsets, uint64_t n_texts, uint32_t unit, ACMRecord *records,
                             uint64_t *char_start, uint32_t *char_len, uint8_t *edge, uint64_t capacity,
                             uint64_t *n_found);   /* blocking */
int acm_scan_chars (ACMachine *machine, const void *text, uint64_t n_symbols, uint32_t unit, ACMRecord *records,
                    uint64_t *char_start, uint32_t *char_len, uint8_t *edge, uint64_t capacity, uint64_t *n_found);

#ifdef __cplusplus
}
#endif
#endif
