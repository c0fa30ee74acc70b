/*
 * acm_gpu.h -- bulk-scan extension of the acm_* API: the MI355X (gfx950) hot path.
 *
 * The reference has no buffer-level entry point: its hot path is the CALLER's loop
 *
 *     for (i = 0; i < n; i++)                                   examples/test.c:17-23
 *       for (j = 0, nb = acm_match (&cursor, &text[i]); j < nb; j++)   aho_corasick.c:434-448
 *         acm_get_match (cursor, j, &holder);                   aho_corasick.c:451-482
 *
 * Every scan function below is DEFINED as that loop started from acm_initiate(machine): it
 * yields one ACMRecord per (i, j) with end_pos = i, length = holder.length and keyword_id = the
 * 0-based rank of the keyword in order of first acm_insert_end_of_keyword (the value
 * machine->nb_sequences had just before aho_corasick.c:352), in the loop's order
 * (end_pos ascending, then j ascending == length descending).
 *
 * The acm_gpu_* functions run on the GPU as hand-written HIP and have NO CPU fallback: a machine
 * they cannot take (symbol size not in {1,2,4,8}; a comparator other than ACM_CMP_DEFAULT unless
 * the plan is made with acm_gpu_plan_create_classes) or a missing device is reported as an error
 * code.  acm_scan, the call on the machine itself, is total over machines: what the
 * GPU cannot take by its nature runs the loop above on the host and says so (acm_scan_path); a
 * missing device is still an error there, never a silent fallback.
 *
 * Plain C ABI: pointers and sizes only.  `stream` arguments are a hipStream_t passed as void *
 * (NULL = the default stream); `d_` pointers are device memory on the plan's device.
 */
#ifndef ACM_GPU_H_AMD
#define ACM_GPU_H_AMD

#include "acm.h"
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Canonical match record, 16 bytes. */
typedef struct {
  uint64_t end_pos;    /* index of the symbol at which the keyword ends */
  uint32_t length;     /* MatchHolder.length of that match */
  uint32_t keyword_id; /* first-insertion rank of the keyword */
} ACMRecord;

enum {
  ACM_GPU_OK = 0,
  ACM_GPU_E_INELIGIBLE = -1, /* comparator is not ACM_CMP_DEFAULT, or symbol size not 1/2/4/8 bytes */
  ACM_GPU_E_NODEVICE = -2,   /* no usable HIP device */
  ACM_GPU_E_HIP = -3,        /* a HIP call failed (message on stderr) */
  ACM_GPU_E_OVERFLOW = -4,   /* more matches than `capacity`; the count output holds the number needed */
  ACM_GPU_E_ARG = -5,        /* invalid argument */
  ACM_GPU_E_NOMEM = -6,
  ACM_GPU_E_INTERNAL = -7,   /* a device-side consistency check failed (never expected) */
  ACM_GPU_E_FORMAT = -8,     /* not a flat-table blob, wrong version, or its contents do not hold together */
  ACM_GPU_E_IO = -9,         /* a file could not be read or written */
  ACM_GPU_E_COMM = -10       /* librccl.so could not be loaded, or an RCCL call failed (message on stderr) */
};
const char *acm_gpu_strerror (int code);
int acm_gpu_device_count (void);

/* Fills `matcher` (initialised with acm_matcher_init, released with acm_matcher_release) with what
 * acm_get_match would have produced for a record of the bulk scan: letters[] = the dictionary's
 * spelling of keyword `keyword_id` (reference aho_corasick.c:472-479), its length and its value
 * (:480).  Host side, no GPU involved. */
int acm_get_keyword (const ACMachine *machine, uint32_t keyword_id, MatchHolder *matcher);

/* ------------------------------------------------------------------ flattened tables (host)
 * Snapshot of the machine's goto / failure / output functions as flat arrays (what
 * struct _ac_state holds per node in the reference: transitions :47, fail_state :53,
 * is_end_of_keyword :54, nb_outputs :55, previous :49-52).  States are renumbered breadth-first
 * (root = 0, children in memcmp order), so shallow -- hot -- states get the small ids and
 * depth(s) is monotone in s.  Needs no GPU. */
typedef struct ACMFlat ACMFlat;

typedef struct {
  uint32_t sym_bytes;   /* 1, 2, 4 or 8 */
  uint32_t n_states;
  uint32_t n_keywords;
  uint32_t n_edges;     /* = n_states - 1 */
  uint32_t lmax;        /* longest keyword, in symbols */
  uint32_t max_outputs; /* max over states of nb_outputs */
  uint32_t alpha_lo;    /* byte alphabets: smallest symbol used by any keyword */
  uint32_t alpha_span;  /* byte alphabets: largest - smallest + 1 (0 for an empty machine) */
  uint32_t width;       /* byte alphabets: dense row width = span + 1 ("other" class last), or 256 */
} ACMFlatInfo;

typedef struct {
  const uint32_t *row_ptr;     /* [n_states + 1] CSR of the goto function */
  const uint32_t *edge_sym;    /* [n_edges] symbol value (little-endian read of sym_bytes bytes), ascending memcmp order per row */
  const uint32_t *edge_next;   /* [n_edges] g(state, symbol) */
  const uint32_t *fail;        /* [n_states] f(state); f(root) = 0 */
  const uint32_t *depth;       /* [n_states] */
  const uint32_t *nb_outputs;  /* [n_states] what acm_match returns in that state */
  const uint32_t *term_kw;     /* [n_states] keyword_id if a keyword ends here, else 0xFFFFFFFF */
  const uint32_t *out_link;    /* [n_states] nearest keyword-terminal state strictly down the failure chain, 0 if none */
  const uint32_t *depth_start; /* [lmax + 2] first state id of each depth; depth_start[lmax + 1] = n_states */
  const uint32_t *kw_state;    /* [n_keywords] terminal state of each keyword */
  /* comparator-class machines only (acm_flatten_classes), else NULL / 0 */
  const uint16_t *class_map;   /* [class_entries] symbol value -> class id: what edge_sym holds, and what the text is mapped through */
  const uint32_t *edge_letter; /* [n_edges] the dictionary's own symbol on each edge (what MatchHolder.letters[] point at) */
  uint32_t class_entries;      /* 256 or 65536 */
  uint32_t n_classes;
  /* 8-byte symbols only, else NULL / 0: the distinct symbols of the dictionary, ascending; edge_sym
   * holds 1 + the index into this table (0 stands for every other symbol a text may hold) */
  const uint64_t *keys64;
  uint32_t n_keys64;
  /* 4-byte symbols flattened over comparator classes only, else NULL / 0: the dictionary's distinct
   * symbols (ascending by value) and their classes 1 .. n_classes (what edge_sym holds; 0 stands
   * for a symbol that compares equal to none of them), and one symbol of each class in comparator
   * order (a text symbol is classified against these when a scan first meets it) */
  const uint32_t *keys32, *keys32_class;
  uint32_t n_keys32;
  const uint32_t *class_rep32;
} ACMFlatView;

int acm_flatten (ACMachine *machine, ACMFlat **out);
/* Machines created with another comparator than ACM_CMP_DEFAULT (aho_corasick.h:33,45; e.g. the
 * case-insensitive alphacmp of generic_test.c:48-54) over symbols of sym_bytes = 1 or 2 bytes: the
 * comparator is called on all 256 / 65,536 symbol values to find the classes of symbols it cannot
 * tell apart; the tables are built over class ids and a plan made from them maps the text through
 * the class table on the device before walking it.  ACM_GPU_E_INELIGIBLE if the comparator is not
 * a consistent order over all values.  (The symbol size is an argument because a custom
 * comparator's cmp_arg is opaque.)
 * sym_bytes = 4 (the reference's own example: wchar_t with the case-insensitive alphacmp,
 * generic_test.c:48-54,62-164): 2^32 values cannot be enumerated, so the classes are those of the
 * dictionary's own symbols; a plan made from such tables classifies the symbols of a text when it
 * first meets them, with the machine's comparator, on the host (ACMFlatView::keys32).  Such tables
 * have no serialised form (acm_flat_to_blob: ACM_GPU_E_ARG). */
int acm_flatten_classes (ACMachine *machine, uint32_t sym_bytes, ACMFlat **out);
void acm_flat_release (ACMFlat *flat);
void acm_flat_info (const ACMFlat *flat, ACMFlatInfo *info);
void acm_flat_view (const ACMFlat *flat, ACMFlatView *view);
/* Failure-resolved (DFA) rows of states [0, n_rows) of a byte-alphabet machine:
 * out[s * width + cls] = delta(s, alpha_lo + cls) | (nb_outputs(next) ? top bit : 0), class
 * `span` (when width == span + 1) standing for every symbol outside [lo, lo + span).
 * entry_bytes is 2 (n_states <= 32768) or 4. */
int acm_flat_dense_rows (const ACMFlat *flat, uint32_t n_rows, uint32_t entry_bytes, void *out);

/* Serialised form of the flat tables (versioned, little-endian; layout in acm_flat.c).  The
 * reference keeps a machine in memory only and rebuilds it from its keywords at every start; a
 * blob restores the scan tables without the keywords or the trie.  Loading recomputes the failure
 * function and every derived array from the goto function and compares: a blob that loads is what
 * acm_flatten would have produced.  Values (`void *` of acm_insert_end_of_keyword) are process-
 * local and not part of a blob; keyword ids and spellings are (acm_flat_keyword). */
size_t acm_flat_blob_bytes (const ACMFlat *flat);
int acm_flat_to_blob (const ACMFlat *flat, void *out, size_t capacity);
int acm_flat_from_blob (const void *blob, size_t bytes, ACMFlat **out);
int acm_flat_save (const ACMFlat *flat, const char *path);
int acm_flat_load (const char *path, ACMFlat **out);
/* Spelling of keyword `keyword_id` from the tables alone -- what MatchHolder.letters[] spell
 * (aho_corasick.c:472-479): min(length, capacity) symbols of sym_bytes bytes each, front to back. */
int acm_flat_keyword (const ACMFlat *flat, uint32_t keyword_id, void *symbols, uint32_t capacity, uint32_t *length);

/* ------------------------------------------------------------------ device plan */
typedef struct ACMPlan ACMPlan;

typedef struct {
  int device;
  uint32_t kernel;       /* 1 = dense-row byte kernel (automaton in LDS); 2 = CSR walk (any symbol size, any
                            alignment); 2- and 4-byte symbols in 16-byte aligned buffers: 4 = start-parallel kernel
                            (root table by symbol value, every position verified independently), or
                            3 = sparse automaton walk when the environment says ACM_GPU_SPARSE=walk;
                            5 = 4-gram sieve kernel: byte dictionaries whose hot rows outgrow LDS (more than about
                            1,300 keywords over a-z) with some keyword of 4 symbols or more
                            (ACM_GPU_GRAM=0: kernel 1 instead, ACM_GPU_GRAM=2: kernel 5 whenever possible) */
  uint32_t entry_bytes;  /* dense entries: 2 or 4 */
  uint32_t width;        /* dense row width */
  uint32_t dense_rows;   /* rows resident in HBM */
  uint32_t lds_rows;     /* states whose failure-resolved row is staged in LDS by every workgroup */
  uint32_t lds_hotfail;  /* further states for which LDS holds the nearest failure-chain state that has a row (2 B each) */
  uint32_t lds_bytes;    /* dynamic LDS per workgroup */
  uint32_t block_threads;
  uint32_t grid_blocks;
  uint32_t chunk_bytes;  /* text bytes per lane-stream per tile */
  uint32_t streams;      /* independent streams per lane */
  uint64_t table_bytes;  /* device bytes held by the plan */
  uint32_t delta_keywords; /* keywords added since the tables were made, held by the delta plan (acm_gpu_plan_update) */
  uint32_t merges;         /* updates that rebuilt the tables (the delta had outgrown its share) */
  uint32_t records_direct; /* 1: the scan kernel writes the 16-byte records itself (kernel 5 on alphabets of at most 29
                              symbols; kernel 2); 0: it parks 8-byte items / hits that a second kernel turns into records */
  uint32_t variant;        /* kernel 5: 2 = scan_gram2_kernel (lane-local sieve on two bits per 4-gram: alphabets of up to
                              26 symbols + "other"; ACM_GPU_GRAM2=0 selects the older form); | 4: the keywords of 1-3 symbols
                              have a pass of their own behind it (scan_short_kernel); | 8: that pass reads the keyword ids
                              from HBM (more of them than LDS holds: about 29 K) */
} ACMPlanInfo;

/* Flattens `machine` and uploads the tables to `device`.  The plan is a snapshot: keywords
 * inserted later are not seen by it until acm_gpu_plan_update.
 * A plan owns scratch buffers that its scans share (item regions, the running record count, the
 * class-mapped / aligned copy of the text): scans of ONE plan must be issued from one host thread
 * and on one stream at a time (consecutive scans on the same stream queue up as usual; for
 * concurrent streams or threads make one plan each -- the tables are a few MB). */
int acm_gpu_plan_create (ACMachine *machine, int device, ACMPlan **out);
int acm_gpu_plan_create_flat (const ACMFlat *flat, int device, ACMPlan **out);
/* acm_flatten_classes + acm_gpu_plan_create_flat: plan of a machine with a custom comparator over
 * 1- or 2-byte symbols.  Scans of such a plan first map the text to class ids (one more pass over
 * the text into a buffer the plan owns), then run the same kernels. */
int acm_gpu_plan_create_classes (ACMachine *machine, uint32_t sym_bytes, int device, ACMPlan **out);
/* Brings a plan up to date with the machine it was made from after keywords were added to it
 * (the reference inserts while it scans: README.md:352-356, generic_test.c:214-229), without
 * rebuilding its tables and without waiting for the device:
 *   - plans of the start-parallel kernel (2- and 4-byte symbols) are edited in place: only the
 *     words of the new keywords' own states change, and they are written on the stream of the next
 *     scan, in front of it.  That next scan (any entry point that scans or walks the plan) is the
 *     one call of such a plan that is NOT only queued: the changed words come from pageable host
 *     memory, in a copy that returns when `stream` has reached it (hipMemcpyWithStream), and the
 *     first update of a plan -- its tables still lie in the blob of its creation -- as well as one
 *     that outgrows the headroom of the tables waits for the whole device
 *     (hipDeviceSynchronize), allocates and sends the tables again.  Every later scan is
 *     asynchronous as its entry point says;
 *   - every other plan keeps its tables; the keywords added since it was made are flattened into a
 *     small delta plan of their own (cost independent of the size of the dictionary), scanned
 *     right after the plan into the same record buffer -- the match set of a dictionary is the
 *     union of its keywords' match sets.  Once the delta holds more than an eighth of the
 *     dictionary (at least 256 keywords) the next update builds one plan of everything again
 *     (that one waits for the device).
 * Not while a stream (acm_gpu_stream_*) is open on the plan.  acm_scan() calls this by itself. */
int acm_gpu_plan_update (ACMPlan *plan, ACMachine *machine);
void acm_gpu_plan_destroy (ACMPlan *plan);
void acm_gpu_plan_info (const ACMPlan *plan, ACMPlanInfo *info);

/* Scan d_text[0 .. n_symbols) from the root state.  Matches whose end index is < emit_from are
 * not reported (warm-up region of a shard: pass the lmax - 1 symbols preceding the shard and
 * emit_from = their number).
 *
 *   end_pos of a match ending at buffer index i  =  pos_base + i
 *
 * Records are appended to d_records in no particular order (at most `capacity`); *d_count
 * (device, 8 bytes) receives the TOTAL number of matches, which may exceed capacity -- nothing is
 * dropped silently: compare and re-run with a larger buffer.  Asynchronous on `stream`. */
int acm_gpu_scan_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from,
                         uint64_t pos_base, ACMRecord *d_records, uint64_t capacity,
                         uint64_t *d_count, void *stream);

/* Sum of acm_match return values over the buffer (reference: generic_test.c:272-273), no records. */
int acm_gpu_count_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from,
                          uint64_t *d_count, void *stream);

/* Puts n records into canonical order (end_pos ascending, length descending) in place, for ANY
 * 64-bit end_pos and ANY 32-bit length: the records need not come from this plan (lengths above
 * its longest keyword, positions with any of the 64 bits set).  Records equal in both fields keep
 * the order they came in.  n must be below 2^31 (ACM_GPU_E_ARG).
 * d_tmp must hold acm_gpu_sort_tmp_bytes(n) bytes.  Asynchronous on `stream`. */
size_t acm_gpu_sort_tmp_bytes (uint64_t n);
int acm_gpu_sort_records_device (ACMPlan *plan, ACMRecord *d_records, uint64_t n, void *d_tmp,
                                 size_t tmp_bytes, void *stream);

/* The same order for records whose end_pos all lie in [pos_lo, pos_lo + span) -- what a scan of
 * `span` symbols with pos_base = pos_lo (and any emit_from) leaves: three passes over the records
 * (position buckets, then sorts of a few thousand records in LDS) instead of the radix sort's
 * twelve.  A range the buckets cannot take (2^40 positions or more) goes to that radix sort, keyed
 * by end_pos - pos_lo: any pos_lo, any span up to 2^64 - 1, any 32-bit length.
 * A record outside the range makes acm_gpu_plan_status report ACM_GPU_E_INTERNAL.
 * d_tmp must hold acm_gpu_order_tmp_bytes(plan, n, span) bytes.  Asynchronous on `stream`. */
size_t acm_gpu_order_tmp_bytes (const ACMPlan *plan, uint64_t n, uint64_t span);
int acm_gpu_order_records_device (ACMPlan *plan, ACMRecord *d_records, uint64_t n, uint64_t pos_lo, uint64_t span,
                                  void *d_tmp, size_t tmp_bytes, void *stream);

/* Records on the wire.  The records of a scan of `span` symbols with pos_base = pos_lo hold
 * positions in [pos_lo, pos_lo + span), lengths up to the plan's lmax and ids below its number of
 * keywords: when that fits 64 bits (acm_gpu_wire_bits returns 0 and the three field widths; config
 * 4's shards: 34 + 4 + 17) a record packs to ONE 8-byte word,
 *     (end_pos - pos_lo) | length << pos_bits | keyword_id << (pos_bits + len_bits),
 * half of what a shard sends to the root in a multi-GPU scan (acm_gpu_multi_* and sharded.py pack
 * behind the canonical order and unpack on the root; the order is kept: index i stays index i).
 * Asynchronous on `stream`; d_packed / d_records on the current device of the call. */
int acm_gpu_wire_bits (const ACMPlan *plan, uint64_t span, uint32_t *pos_bits, uint32_t *len_bits, uint32_t *kw_bits);
int acm_gpu_pack_records_device (const ACMRecord *d_records, uint64_t n, uint64_t pos_lo, uint32_t pos_bits, uint32_t len_bits,
                                 uint64_t *d_packed, void *stream);
int acm_gpu_unpack_records_device (const uint64_t *d_packed, uint64_t n, uint64_t pos_lo, uint32_t pos_bits, uint32_t len_bits,
                                   ACMRecord *d_records, void *stream);

/* acm_gpu_scan_device and the canonical order of what it found in ONE call that only queues work on
 * `stream`: the order passes read the number of records from *d_count on the device, so no host
 * round trip separates the scan from them (the caller loop of aho_corasick.h:47,77 yields its
 * matches in this order; this is that loop's output, complete, with one synchronisation at the
 * end).  d_records[0 .. *d_count) is in canonical order afterwards when *d_count <= capacity; a
 * scan that overflowed leaves the total in *d_count and nothing in order (repeat it with room).
 * Plans of big byte dictionaries (the 4-gram kernel, narrow alphabets, keywords of up to 1,024
 * symbols, no pending delta) scan in tiles into d_tmp and put the records in order in ONE pass
 * over them; every other plan scans as acm_gpu_scan_device does and runs
 * acm_gpu_order_records_device's passes behind it.  Same records, same order either way.
 * d_tmp must hold acm_gpu_scan_ordered_tmp_bytes(plan, capacity, n_symbols) bytes (about
 * 16 bytes per record of capacity, plus a few megabytes). */
size_t acm_gpu_scan_ordered_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols);
int acm_gpu_scan_ordered_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from,
                                 uint64_t pos_base, ACMRecord *d_records, uint64_t capacity, uint64_t *d_count,
                                 void *d_tmp, size_t tmp_bytes, void *stream);

/* Host-buffer convenience: upload, scan, sort, download; blocking.  On ACM_GPU_E_OVERFLOW
 * *n_found holds the capacity needed. */
int acm_gpu_scan_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t emit_from,
                       uint64_t pos_base, ACMRecord *records, uint64_t capacity, uint64_t *n_found);

/* The bulk call on the machine itself, for EVERY machine the reference's API can make
 * (aho_corasick.h:33-45: any comparator, any symbol): the records of the caller's loop over
 * text[0 .. n_symbols), in the loop's order.  Keeps a plan cached inside the machine and brings it
 * up to date when the dictionary changed since the last call.  Device = $ACM_GPU_DEVICE or 0.
 *   - ACM_CMP_DEFAULT over 1, 2, 4 or 8 byte symbols: the GPU scan (ACM_SCAN_PATH_GPU);
 *   - another comparator: the library cannot know the symbol size (letters are opaque pointers), so
 *     the caller says it once with acm_set_symbol_bytes.  1, 2 or 4 bytes: the GPU scan over the
 *     comparator's symbol classes (acm_gpu_plan_create_classes; ACM_SCAN_PATH_GPU_CLASSES) -- the
 *     reference's own example, wchar_t + alphacmp (examples/aho_corasick_generic_test.c:48-54), runs
 *     this way.  Any other size, or a comparator that is no consistent order over all symbol values
 *     (acm_flatten_classes refuses it): the loop itself, on the host, with this library's own
 *     acm_match / acm_get_match steps (ACM_SCAN_PATH_CPU_LOOP) -- SURVEY.md 8(b): "otherwise it runs
 *     loop a9 on the CPU".  Without acm_set_symbol_bytes such a machine is ACM_GPU_E_INELIGIBLE.
 * A missing device or a failing HIP call is an ERROR for the machines of the first two kinds
 * (ACM_GPU_E_NODEVICE, ACM_GPU_E_HIP): the GPU path never falls back to the host silently.
 * acm_scan_path says which of the three the machine's last acm_scan ran. */
#define ACM_SCAN_PATH_NONE 0
#define ACM_SCAN_PATH_GPU 1
#define ACM_SCAN_PATH_GPU_CLASSES 2
#define ACM_SCAN_PATH_CPU_LOOP 3
int acm_scan (ACMachine *machine, const void *text, uint64_t n_symbols, ACMRecord *records,
              uint64_t capacity, uint64_t *n_found);
int acm_set_symbol_bytes (ACMachine *machine, uint32_t sym_bytes);
int acm_scan_path (const ACMachine *machine);

/* ------------------------------------------------------------------ batch scan: many texts in one call
 * The reference's callers mostly do not have one text: they run the loop above word by word and
 * line by line (log lines, packets, table cells), each from acm_initiate on its own.  A batch is
 * n_texts such texts packed into one buffer: text t is the symbols [offsets[t], offsets[t + 1]),
 * with offsets[0 .. n_texts] non-decreasing, offsets[0] = 0 and offsets[n_texts] = n_symbols (empty
 * texts are allowed).
 *
 * The result is DEFINED as the caller loop run from acm_initiate(machine) on every text separately,
 * t = 0, 1, ..., the results concatenated; a record of text t carries end_pos = offsets[t] + i, the
 * index in the whole buffer.  Positions are therefore unique and the order is the plain canonical
 * one (end_pos ascending, length descending).  Beside the records:
 *     text_id[r]            the text of record r;
 *     first[0 .. n_texts]   records [first[t], first[t + 1]) are those of text t, first[n_texts] is
 *                           the number of records; end_pos - offsets[text_id] is the position
 *                           inside the text.
 * (Scanning the concatenation with acm_gpu_scan_* instead would also report the matches that begin
 * in one text and end in the next.  The automaton reports every occurrence of every keyword, so
 * the batch's records are exactly the concatenation's that lie inside one text: the ordered scan of
 * the buffer -- whatever kernel the plan has -- and one pass over its RECORDS, dev_batch.h.)
 *
 * acm_gpu_scan_batch_device: acm_gpu_scan_ordered_device (emit_from = 0, pos_base = 0) and that pass
 * behind it on `stream`; asynchronous to exactly the extent that call is.  CAPACITY: `capacity`
 * must hold the matches of the CONCATENATION (they are found first, in d_tmp).  *d_count <=
 * capacity afterwards: it is the exact number of the batch's records, and d_records, d_text_id and
 * d_first are complete.  *d_count > capacity: it is the concatenation's count -- a capacity that is
 * guaranteed to suffice -- and the three outputs are unspecified; nothing is dropped silently.
 * n_texts = 0 requires n_symbols = 0 and gives no record; n_texts >= 2^32 is ACM_GPU_E_ARG, and so is
 * capacity >= 2^31 (the tiles' counts and their prefix sum are 32-bit, as the bucket order's are).
 * d_offsets that break the contract above leave *d_count = 0 and make acm_gpu_plan_status report
 * ACM_GPU_E_INTERNAL (as a record out of range does in acm_gpu_order_records_device); nothing is
 * read or written out of bounds.  d_tmp must hold acm_gpu_scan_batch_tmp_bytes(plan, capacity,
 * n_symbols, n_texts) bytes (about 32 bytes per record of capacity, 4 bytes per 4,096 symbols).
 * acm_gpu_scan_batch_host: the same from host memory, blocking; offsets[] is checked on the host
 * (ACM_GPU_E_ARG); on ACM_GPU_E_OVERFLOW *n_found holds a capacity that suffices.
 * acm_scan_batch: the call on the machine itself, total over machines exactly as acm_scan is (same
 * paths, same cached plan, acm_scan_path says which ran): the GPU paths run
 * acm_gpu_scan_batch_host, ACM_SCAN_PATH_CPU_LOOP runs the loop on the host from the root at every
 * offset.  A missing device stays an error, never a fallback.
 * text_id and first may be NULL wherever they appear. */
size_t acm_gpu_scan_batch_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_batch_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols,
                               const uint64_t *d_offsets, uint64_t n_texts,
                               ACMRecord *d_records, uint32_t *d_text_id /* may be NULL */,
                               uint64_t *d_first /* n_texts + 1, may be NULL */,
                               uint64_t capacity, uint64_t *d_count,
                               void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_batch_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                             ACMRecord *records, uint32_t *text_id, uint64_t *first,
                             uint64_t capacity, uint64_t *n_found);          /* blocking */
int acm_scan_batch (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
                    ACMRecord *records, uint32_t *text_id, uint64_t *first,
                    uint64_t capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ flow scans: batch texts that continue earlier ones
 * The reference's scan state is the caller's cursor: one `const ACState *` per connection, file or
 * log source, fed a piece whenever one arrives, and a keyword cut by a piece boundary is still found
 * (aho_corasick.h:47-48,70).  An ACMFlows holds that state for n_flows flows on the plan's device:
 * per flow its CARRY, the last min (lmax - 1, symbols seen so far) symbols in the caller's symbol
 * size, and the carry's length -- a spelling, not a state id, so it is valid for every plan kind,
 * for class and interned plans and for a plan with a delta (lmax is the larger of the two).
 *
 * acm_gpu_flows_create: all flows at the root.  The slot width is fixed here (lmax - 1 symbols,
 * rounded up to whole 16 bytes); when a later acm_gpu_plan_update brings a keyword the slots cannot
 * serve, the next flow scan returns ACM_GPU_E_ARG -- it never scans with a short carry.
 * acm_gpu_flows_reset: the flows d_flow_ids[0 .. n) (device memory; NULL: all of them) back to the
 * root, on `stream`.  Destroy the flows before their plan.
 *
 * A flow scan is a batch scan (above: same buffer, offsets[] contract, text_id, first, d_count and
 * capacity rule) whose text t continues flow f = d_flow[t] (d_flow NULL: text t is flow t, n_texts
 * <= n_flows).  DEFINITION: let H_f be everything flow f was fed since its creation or reset; text
 * t yields the records of the caller loop run from the root over H_f followed by text t that END
 * INSIDE text t, with end_pos = offsets[t] + the index inside text t -- so `length` may exceed the
 * position inside the text.  Plain canonical order.  Afterwards H_f has grown by text t.  Empty
 * texts leave their flow as it is, flows that do not appear are untouched.
 * Every flow id must be below n_flows and no flow may appear twice in one call.  On the device a
 * violation is handled as bad offsets are: *d_count = 0, acm_gpu_plan_status reports
 * ACM_GPU_E_INTERNAL, nothing is read or written out of bounds and NO carry changes; the host entry
 * checks the same on the host (ACM_GPU_E_ARG).
 * CAPACITY must hold the matches of the scanned buffer, which is the texts with their carries in
 * front (dev_flows.h).  *d_count > capacity: it is a capacity that suffices, the outputs are
 * unspecified and no carry has changed: the same call is simply repeated with room.
 * d_tmp must hold acm_gpu_scan_flows_tmp_bytes (...) bytes: the batch scan's scratch for the WORST
 * CASE of n_symbols + n_texts * (lmax - 1) symbols plus that many symbols (the texts are copied
 * behind their carries once) and 20 bytes per text.  n_texts and capacity must be below 2^31.
 * acm_gpu_scan_flows_device is nothing but launches on `stream`; one call at a time per ACMFlows
 * and per plan.  acm_gpu_scan_flows_host: the same from host memory, blocking (offsets[n_texts] must
 * equal n_symbols); ACM_GPU_E_OVERFLOW leaves a capacity that suffices in *n_found. */
typedef struct ACMFlows ACMFlows;
int acm_gpu_flows_create (ACMPlan *plan, uint64_t n_flows, ACMFlows **out);
void acm_gpu_flows_destroy (ACMFlows *flows);
int acm_gpu_flows_reset (ACMFlows *flows, const uint32_t *d_flow_ids /* NULL: all */, uint64_t n, void *stream);
size_t acm_gpu_scan_flows_tmp_bytes (const ACMPlan *plan, const ACMFlows *flows, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_flows_device (ACMPlan *plan, ACMFlows *flows, const void *d_text, uint64_t n_symbols,
                               const uint64_t *d_offsets, const uint32_t *d_flow /* [n_texts], NULL: text t is flow t */,
                               uint64_t n_texts, ACMRecord *d_records, uint32_t *d_text_id /* may be NULL */,
                               uint64_t *d_first /* n_texts + 1, may be NULL */, uint64_t capacity, uint64_t *d_count,
                               void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_flows_host (ACMPlan *plan, ACMFlows *flows, const void *text, uint64_t n_symbols,
                             const uint64_t *offsets, const uint32_t *flow /* NULL: text t is flow t */, uint64_t n_texts,
                             ACMRecord *records, uint32_t *text_id, uint64_t *first,
                             uint64_t capacity, uint64_t *n_found);          /* blocking */

/* The cursor on the machine: acm_scan continued from *cursor, the reference's own `const ACState *`
 * (acm_initiate gives the root's).  Returns the records of the caller loop continued from *cursor
 * over text[0 .. n_symbols), end_pos = the index in `text` (so `length` may exceed end_pos + 1);
 * *cursor afterwards is exactly the state the per-symbol loop would hold, usable with acm_match and
 * acm_get_match at once -- bulk and per-symbol feeding mix freely.  Same three paths as acm_scan
 * (acm_scan_path says which ran).  On any error, ACM_GPU_E_OVERFLOW included, *cursor is unchanged. */
int acm_scan_from (ACMachine *machine, const ACState **cursor, const void *text, uint64_t n_symbols,
                   ACMRecord *records, uint64_t capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ per-keyword tallies
 * What the reference's callers do with their matches above all: count how often every keyword occurs
 * (examples/aho_corasick_generic_test.c:168-210 runs `(*(size_t *) m3.value)++` for every match; the
 * README's timings are for "find (and count occurencies of) those keywords").  The answer is one
 * counter per keyword; no record leaves the device and no record capacity for the whole text has to
 * be guessed.
 *
 * DEFINITION: tally[k] grows by the number of records of the caller loop over text[0 .. n_symbols)
 * with keyword_id == k and end_pos >= emit_from; `total` is their number -- what acm_gpu_count_device
 * reports, and the sum of the increments.  The counters are ADDED TO, never cleared: a caller zeroes
 * them once and then feeds many texts (as the reference's `value`s keep counting).
 *
 * acm_gpu_tally_device: the text is cut into windows of window_symbols symbols (a multiple of 16,
 * greater than 0).  Window w owns the matches that END in it; its scan starts from the root lmax - 1
 * symbols earlier (lmax: the larger of the plan's and its delta's), rounded down to a 16-byte
 * boundary of the text -- acm_gpu_multi_shard_bounds' rule.  Windows that lie wholly in front of
 * emit_from are skipped.  Every window is scanned as acm_gpu_scan_device scans (any plan kind, a
 * pending delta included) into `capacity` records inside d_tmp and tallied there (dev_tally.h).
 * CAPACITY is per WINDOW, greater than 0 and below 2^31.  A window of W symbols has at most W x M
 * records, M = the sum of the plan's and its delta's ACMFlatInfo::max_outputs: capacity >=
 * window_symbols x M cannot overflow.  Outputs, all device memory, valid when `stream` has passed:
 *     no window found more than `capacity` records:  d_tally[k] += the increments, *d_total = their
 *         sum, *d_need = the largest record count of a window (<= capacity);
 *     some window did:  d_tally is left EXACTLY as it was (all or nothing: the counters accumulate
 *         over calls, an overflowing call must not leave half a text in them), *d_total = 0,
 *         *d_need = the largest record count of a window (> capacity): a capacity that suffices for
 *         this window size.
 * n_keywords = the entries of d_tally, at least the number of keywords the plan and its delta report
 * (acm_gpu_tally_keywords: acm_nb_keywords of the machine when the plan was made or last updated),
 * else ACM_GPU_E_ARG.
 * d_tmp must hold acm_gpu_tally_tmp_bytes (plan, window_symbols, capacity) bytes (16 per record of
 * capacity, 8 per keyword).  The call only queues work on `stream`; one scan at a time per plan as
 * ever, and not while a stream (acm_gpu_stream_*) is open on it.  A keyword id in a record that is
 * no keyword of the plan (never expected) is not counted and makes acm_gpu_plan_status report
 * ACM_GPU_E_INTERNAL.
 * acm_gpu_tally_form: which of dev_tally.h's two kernel forms the plan's tallies take -- counters in
 * LDS for dictionaries of up to 16,384 keywords, global atomics beyond that or when the environment
 * says ACM_GPU_TALLY=global.
 * acm_gpu_tally_host: the same from host memory, blocking, emit_from = 0.  It picks the window and
 * the capacity itself: windows of 32 Mi symbols and room for 2 Mi records (32 MiB; less for a text
 * that cannot have that many; ACM_GPU_TALLY_CAPACITY=<records> in the environment sets another room).
 * It never returns ACM_GPU_E_OVERFLOW: when a window held more, the call is repeated once with
 * window_symbols = capacity / M rounded down to a multiple of 16 (the capacity grown to 16 x M when
 * that would be 0), which cannot overflow by the bound above.  `total` may be NULL.
 * acm_tally: the call on the machine itself, total over machines exactly as acm_scan is (same three
 * paths, same cached plan and acm_gpu_plan_update, acm_scan_path says which ran): the GPU paths run
 * acm_gpu_tally_host, ACM_SCAN_PATH_CPU_LOOP runs the caller loop on the host and increments the
 * counters there.  A missing device stays an error, never a fallback.  acm_get_keyword turns an
 * index of `tally` back into the keyword's spelling and value. */
#define ACM_GPU_TALLY_FORM_LDS 1
#define ACM_GPU_TALLY_FORM_GLOBAL 2
size_t acm_gpu_tally_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity);
int acm_gpu_tally_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from,
                          uint64_t *d_tally, uint64_t n_keywords,
                          uint64_t window_symbols, uint64_t capacity,
                          uint64_t *d_total, uint64_t *d_need,
                          void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_tally_form (const ACMPlan *plan);
uint64_t acm_gpu_tally_keywords (const ACMPlan *plan);
int acm_gpu_tally_host (ACMPlan *plan, const void *text, uint64_t n_symbols,
                        uint64_t *tally, uint64_t n_keywords, uint64_t *total);   /* blocking */
int acm_tally (ACMachine *machine, const void *text, uint64_t n_symbols,
               uint64_t *tally, uint64_t n_keywords, uint64_t *total);

/* ------------------------------------------------------------------ leftmost-longest non-overlapping matches
 * Search-and-replace, redaction, tokenising against a vocabulary and highlighting need ONE tiling of
 * the text, not every occurrence: the non-overlapping matches, taken leftmost first and longest at a
 * tie.  On `ushers` with {he, she, his, hers} the caller loop reports she, he and hers; a replacer
 * acts on `she` alone.
 *
 * DEFINITION.  Let R be a record set; a record's start is end_pos + 1 - length.  SELECT (R):
 *     1. set p to the smallest position;
 *     2. among the records with start >= p take those with the smallest start;
 *     3. of those take the one with the greatest length (two of equal start and length are not
 *        expected -- no scan gives them; the host helper then takes the smaller keyword_id);
 *     4. emit the record;
 *     5. set p to its end_pos + 1;
 *     6. repeat from 2 until no record has start >= p.
 * The output is in canonical order: starts and ends both ascend, no two emitted records share a
 * symbol.  The batch scan's records never cross a text boundary, so SELECT of a batch's records is
 * the concatenation of SELECT of every text's records.
 *
 * acm_select_records: SELECT of records[0 .. n), which are in canonical order, in place in the front
 * of the array; returns the selected count.  The plain sequential pass on the host, no device.
 * Starts are taken as signed numbers (a record of acm_scan_from may begin in front of its text).
 *
 * acm_gpu_select_records_device: the same on the device (dev_select.h).  d_records is in canonical
 * order; d_n (device, may be NULL) holds the record count and n_or_capacity the room of d_records
 * and d_out -- with d_n NULL n_or_capacity is the count itself.  Every position, the starts
 * included, lies in [pos_lo, pos_lo + span), and no length exceeds the plan's lmax (the larger of
 * the plan's and its delta's).  d_out may be d_records, d_count may be d_n.  *d_count (device)
 * receives the selected count; when *d_n exceeds n_or_capacity (a scan that overflowed) nothing is
 * selected and *d_count = *d_n.  The call only queues launches on `stream`, with no host round trip
 * (except for record sets the bucket order does not take -- a span of 2^40 positions or more --
 * where the count comes to the host once, as in acm_gpu_scan_ordered_device).  A record that breaks
 * the contract -- a start below pos_lo (a flow's record that reaches back into its carry, hand-made
 * input), a position outside the range, a length of 0 or beyond lmax -- is DROPPED, nothing is read
 * or written out of bounds and acm_gpu_plan_status reports ACM_GPU_E_INTERNAL, as for a record out
 * of range in acm_gpu_order_records_device.  n_or_capacity must be below 2^31 (ACM_GPU_E_ARG).
 * d_tmp must hold acm_gpu_select_tmp_bytes (plan, n_or_capacity, span) bytes (about 40 bytes per
 * record of capacity).
 * acm_gpu_select_form: which of dev_select.h's two forms the plan's selections take -- tiles of T
 * candidates in LDS (T = 1,024; ACM_GPU_SELECT_TILE=<8 .. 2048> in the environment sets another,
 * read at every call) when lmax <= T, else, or when the environment says ACM_GPU_SELECT=walk, one
 * lane that walks the chain through global memory: slow and correct, so that no plan is refused.
 *
 * acm_gpu_scan_select_device: acm_gpu_scan_ordered_device with emit_from = 0 and the pass above
 * behind it on `stream`.  The selection of a shard is not the shard of the selection: there is no
 * emit_from, and multi-GPU selection is out of scope (select on one device, or gather the records
 * with acm_gpu_multi_* and select them there).  CAPACITY is the batch scan's rule: `capacity` must
 * hold ALL matches, they are found first.  *d_count <= capacity afterwards: it is the exact selected
 * count and d_records is complete.  *d_count > capacity: it is the scan's count -- a capacity that
 * suffices -- and the records are unspecified.  d_tmp must hold acm_gpu_scan_select_tmp_bytes (plan,
 * capacity, n_symbols) bytes.
 * acm_gpu_scan_select_host: the same from host memory, blocking; on ACM_GPU_E_OVERFLOW *n_found holds
 * a capacity that suffices.
 * acm_select: the call on the machine itself, total over machines exactly as acm_scan is (same three
 * paths, same cached plan and acm_gpu_plan_update, acm_scan_path says which ran): the GPU paths run
 * acm_gpu_scan_select_host, ACM_SCAN_PATH_CPU_LOOP runs the caller loop on the host and then
 * acm_select_records.  A missing device stays an error, never a fallback. */
#define ACM_GPU_SELECT_FORM_TILED 1
#define ACM_GPU_SELECT_FORM_WALK 2
uint64_t acm_select_records (ACMRecord *records, uint64_t n);
size_t acm_gpu_select_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t span);
int acm_gpu_select_records_device (ACMPlan *plan, const ACMRecord *d_records, uint64_t n_or_capacity,
                                   const uint64_t *d_n /* device count, may be NULL: n is the count */,
                                   uint64_t pos_lo, uint64_t span, ACMRecord *d_out, uint64_t *d_count,
                                   void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_select_form (const ACMPlan *plan);
size_t acm_gpu_scan_select_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols);
int acm_gpu_scan_select_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                ACMRecord *d_records, uint64_t capacity, uint64_t *d_count,
                                void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_select_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                              ACMRecord *records, uint64_t capacity, uint64_t *n_found);   /* blocking */
int acm_select (ACMachine *machine, const void *text, uint64_t n_symbols, ACMRecord *records,
                uint64_t capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ search-and-replace
 * What a replacer or a redactor does with the selection above: the text with every selected match
 * replaced by its keyword's replacement (or masked), built where the text is -- no record and no
 * byte of the text goes through the host when the pipeline stays on the device.
 *
 * DEFINITION.  Let S = r_0 ... r_{m-1} be a selection: records in canonical order, no two sharing a
 * symbol, every start s_j = end_pos_j + 1 - length_j - pos_base and every end e_j = end_pos_j -
 * pos_base in [0, n_symbols).  Let repl_data, repl_off[0 .. n_keywords] be a replacement table: its
 * symbols have the CALLER's symbol size, the one d_text has (also for class plans and for plans that
 * intern 8-byte symbols); repl_off never decreases and repl_off[0] = 0; the replacement R (k) of
 * keyword k is the symbols [repl_off[k], repl_off[k + 1]) of repl_data and may be empty (deletion).
 * REPLACE (text, S, table) is
 *     text[0 .. s_0)  R (kw_0)  text[e_0 + 1 .. s_1)  R (kw_1)  ...  R (kw_{m-1})  text[e_{m-1} + 1 .. n_symbols)
 * The stretches between the matches are the caller's original symbols, bit for bit -- never the
 * class-mapped or interned copy a plan keeps for its scan.
 * MASK mode: repl_off == NULL, and repl_data points at ONE symbol.  Every symbol of every selected
 * match becomes that symbol; the output has n_symbols symbols.
 * Beside the output: out_symbols, its length; n_replaced = m; and out_start[j] (optional), the index
 * in the output at which replacement j begins -- with r_j the offset map a highlighter or a later pass
 * needs:  out_start[j] = s_j + the sum over i < j of (|R (kw_i)| - length_i), in signed 64-bit
 * arithmetic.
 *
 * acm_replace_records: the plain sequential pass on the host, no device; any sym_bytes > 0.  `n` is
 * the number of records.  ACM_GPU_E_OVERFLOW with *out_symbols = the length needed when out_capacity
 * (symbols) is too small: nothing is written then.  ACM_GPU_E_ARG for records that are no tiling of
 * [pos_base, pos_base + n_symbols) (out of range, overlapping, out of order) and, in table mode, for
 * a keyword id >= n_keywords or a keyword whose repl_off decreases.
 *
 * acm_gpu_replace_records_device: the same on the device (dev_replace.h) for ANY selection resident
 * there -- acm_gpu_scan_select_device's, acm_gpu_select_records_device's, a batch scan's records
 * after selection (they never cross a text).  Arguments in this order: the text (d_text, n_symbols,
 * pos_base), the selection (d_sel, n_or_capacity, d_n: exactly as in acm_gpu_select_records_device --
 * with d_n NULL n_or_capacity is the count itself, else *d_n is the count and n_or_capacity the room;
 * below 2^31), the table (d_repl_data, d_repl_off -- NULL for mask mode --, n_keywords), the output
 * (d_out, out_capacity in symbols, d_out_symbols: device, 8 bytes; d_out_start: device, an int64_t
 * per record of n_or_capacity, may be NULL), the scratch (d_tmp of acm_gpu_replace_tmp_bytes (plan,
 * n_or_capacity, n_symbols) bytes: about 8 per record) and the stream.  The call only queues
 * launches on `stream`, with no host round trip.  d_out must not overlap d_text (ACM_GPU_E_ARG); both
 * may have ANY byte alignment that is a multiple of the symbol size (the copy loads whole aligned
 * 16-byte words of its sources: up to 15 bytes in front of and behind a stretch it copies are read,
 * never beyond the aligned word that holds a byte of the stretch).  *d_out_symbols > out_capacity
 * afterwards: it is the capacity needed, d_out is unspecified and nothing was written outside
 * d_out[0 .. out_capacity).  *d_n > n_or_capacity (a scan that overflowed): *d_out_symbols = 0 and
 * d_out is untouched.  A contract violation -- a record out of range, two records that overlap or
 * are out of order, in table mode a keyword id >= n_keywords or a repl_off that decreases -- is
 * handled as bad offsets and bad records are elsewhere: a validation pass sees every record and the
 * whole table before any address is formed from them, acm_gpu_plan_status reports
 * ACM_GPU_E_INTERNAL, *d_out_symbols = 0, d_out is untouched and nothing is read or written out of
 * bounds.  The output is built in tiles of 16,384 bytes (ACM_GPU_REPLACE_TILE=<bytes> in the
 * environment sets another: a multiple of 16 from 256 to 1 Mi, read at every call).
 *
 * acm_gpu_scan_replace_device: acm_gpu_scan_select_device with the passes above behind it on
 * `stream`; the selected records stay in d_records[0 .. *d_count).  The record capacity rule is
 * select's: `capacity` must hold ALL matches.  *d_count > capacity afterwards: it is the scan's
 * count, *d_out_symbols = 0 and d_out is untouched.  In table mode n_keywords must be at least
 * acm_gpu_tally_keywords (plan), else ACM_GPU_E_ARG.  d_tmp (never NULL) must hold
 * acm_gpu_scan_replace_tmp_bytes (plan, capacity, n_symbols) bytes: the scan's and the selection's
 * scratch is reused, the selection has ended when the replace passes begin.
 * acm_gpu_scan_replace_host: the same from host memory, blocking.  The caller gives NO record
 * capacity: the call counts the matches first (acm_gpu_count_device) and sizes the record room by
 * that; it never reports a record overflow, ACM_GPU_E_OVERFLOW means only "out_capacity is too
 * small, *out_symbols suffices" (n_replaced is valid then, `out` is not).  A text with 2^31 matches
 * or more is ACM_GPU_E_ARG (acm_gpu_scan_select_device's limit: replace such a text in pieces).
 * In table mode n_keywords below acm_gpu_tally_keywords (plan), or a repl_off that decreases or
 * does not begin with 0, is ACM_GPU_E_ARG.  n_replaced may be NULL.
 * acm_replace: the call on the machine itself, total over machines exactly as acm_scan is (same three
 * paths, same cached plan and acm_gpu_plan_update, acm_scan_path says which ran -- recorded on
 * success and on an output overflow): the GPU paths run acm_gpu_scan_replace_host,
 * ACM_SCAN_PATH_CPU_LOOP runs the caller loop on the host into a record room the call grows itself,
 * then acm_select_records, then acm_replace_records.  On every path a table with n_keywords below
 * the machine's number of keywords is ACM_GPU_E_ARG, whether a keyword without an entry matched or
 * not; a record room that cannot be allocated is ACM_GPU_E_NOMEM.  A missing device stays an error,
 * never a fallback. */
int acm_replace_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base,
                         const ACMRecord *records, uint64_t n,
                         const void *repl_data, const uint64_t *repl_off, uint64_t n_keywords,
                         void *out, uint64_t out_capacity, uint64_t *out_symbols);
size_t acm_gpu_replace_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_symbols);
int acm_gpu_replace_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                    const ACMRecord *d_sel, uint64_t n_or_capacity,
                                    const uint64_t *d_n /* device count, may be NULL: n is the count */,
                                    const void *d_repl_data, const uint64_t *d_repl_off /* NULL: mask mode */,
                                    uint64_t n_keywords, void *d_out, uint64_t out_capacity,
                                    uint64_t *d_out_symbols, int64_t *d_out_start /* may be NULL */,
                                    void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_replace_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols);
int acm_gpu_scan_replace_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                 ACMRecord *d_records, uint64_t capacity, uint64_t *d_count,
                                 const void *d_repl_data, const uint64_t *d_repl_off, uint64_t n_keywords,
                                 void *d_out, uint64_t out_capacity, uint64_t *d_out_symbols,
                                 int64_t *d_out_start, void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_replace_host (ACMPlan *plan, const void *text, uint64_t n_symbols,
                               const void *repl_data, const uint64_t *repl_off, uint64_t n_keywords,
                               void *out, uint64_t out_capacity, uint64_t *out_symbols,
                               uint64_t *n_replaced);   /* blocking */
int acm_replace (ACMachine *machine, const void *text, uint64_t n_symbols,
                 const void *repl_data, const uint64_t *repl_off, uint64_t n_keywords,
                 void *out, uint64_t out_capacity, uint64_t *out_symbols, uint64_t *n_replaced);

/* ------------------------------------------------------------------ tokenising against a vocabulary
 * What a model-side consumer does with the selection: the MaxMatch (greedy longest-match) tokeniser
 * over the dictionary.  A sequence of token ids that covers the text -- one id per selected match and
 * something defined for the symbols no keyword covers --, where every token lies, and for a batch a
 * row pointer per text: a ragged tensor, made where the text is.
 *
 * DEFINITION.  Inputs: text[0 .. n_symbols) in the caller's symbols; a selection S exactly as REPLACE
 * takes it (records in canonical order, no two sharing a symbol, every start s_j = end_pos_j + 1 -
 * length_j - pos_base and every end e_j = end_pos_j - pos_base in [0, n_symbols)); optionally a batch,
 * offsets[0 .. n_texts] under the batch contract (offsets[n_texts] = n_symbols, empty texts allowed;
 * offsets == NULL: the buffer is one text, n_texts is ignored) -- no record crosses a text boundary;
 * optionally tok_of[0 .. n_keywords), the vocabulary id of every keyword (NULL: the token of keyword
 * k is k); gap_base; and a mode.
 * Symbol i is COVERED when some r_j has s_j <= i <= e_j, else UNCOVERED.  The token stream, left to
 * right, has one token per unit:
 *     every selected match: id = tok_of[kw_j] (kw_j without a table), start s_j, length length_j;
 *     ACM_TOKENS_GAP_SYMBOL (0): every uncovered symbol i is a unit of its own, id = gap_base + the
 *         value of text[i] (byte fallback), start i, length 1.  The value is the little-endian read
 *         of the CALLER's symbol, bit for bit, never the class-mapped or interned copy a plan keeps
 *         (acm_replace's rule): under a case-folding comparator an uncovered `U` is gap_base + 'U'.
 *         Only for symbols of 1 or 2 bytes, with gap_base <= 2^32 - 2^(8 x sym_bytes); anything else
 *         is ACM_GPU_E_ARG;
 *     ACM_TOKENS_GAP_RUN (1): every maximal run of uncovered symbols that lies inside ONE text is one
 *         unit, id = gap_base (the "unknown" id), start = the run's first symbol, length = the run's
 *         length (a run of 2^32 symbols or more reports 2^32 - 1); a run that meets a text boundary
 *         is cut there;
 *     ACM_TOKENS_GAP_DROP (2): uncovered symbols give no token.
 * Outputs: tok_id[] (uint32_t); tok_start[] (uint64_t, in the records' coordinate: buffer index +
 * pos_base; optional); tok_len[] (uint32_t; optional); n_tokens; for a batch tok_first[0 .. n_texts]
 * (uint64_t; optional): tokens [tok_first[t], tok_first[t + 1]) are those of text t, tok_first[0] = 0,
 * tok_first[n_texts] = n_tokens, an empty text has an empty range.  Starts ascend strictly; in SYMBOL
 * and RUN mode the tokens tile the buffer: the sum of tok_len is n_symbols.
 * `ushers` with he=0, she=1, his=2, hers=3 (SELECT gives `she`, symbols 1 to 3), gb = gap_base:
 *     SYMBOL  ids [gb+'u', 1, gb+'r', gb+'s']  starts [0, 1, 4, 5]  lengths [1, 3, 1, 1]
 *     RUN     ids [gb, 1, gb]                  starts [0, 1, 4]     lengths [1, 3, 2]
 *     DROP    ids [1]                          starts [1]           lengths [3]
 * The same symbols as the batch `us` | `hers` (offsets 0, 2, 6): SELECT keeps `hers`; RUN gives ids
 * [gb, 3], starts [0, 2], lengths [2, 4], tok_first [0, 1, 2].  `abcd` without a match as the batch
 * `ab` | `cd`: RUN gives two tokens [gb, gb] at 0 and 2; as one text it gives one.
 *
 * acm_tokens_records: the plain sequential pass on the host, no device; any sym_bytes > 0 in RUN and
 * DROP mode (the text is not read there and may be NULL).  `n` is the number of records.  tok_id,
 * tok_start, tok_len and tok_first may each be NULL; tok_id == NULL: the call only counts and ignores
 * token_capacity; tok_first without offsets is ACM_GPU_E_ARG.  ACM_GPU_E_OVERFLOW when token_capacity
 * is too small: *n_tokens = the count needed, nothing is written to the three token arrays, tok_first
 * is written all the same.  ACM_GPU_E_ARG for records that are no tiling (REPLACE's rule), a record
 * that crosses a text boundary, a keyword_id >= n_keywords when tok_of is given, offsets that break
 * the batch contract, a mode above 2, the SYMBOL-mode limits above and n_texts >= 2^31.
 *
 * acm_gpu_tokens_records_device: the same on the device (dev_tokens.h) for ANY selection resident
 * there.  Arguments in this order: the text (d_text, n_symbols, pos_base), the selection (d_sel,
 * n_or_capacity below 2^31, d_n: exactly acm_gpu_replace_records_device's), the batch (d_offsets --
 * NULL: one text, d_tok_first must then be NULL too --, n_texts below 2^31), the vocabulary (d_tok_of
 * or NULL, n_keywords, gap_base, mode), the outputs (d_tok_id, d_tok_start, d_tok_len, token_capacity,
 * d_n_tokens: device, 8 bytes; d_tok_first), the scratch and the stream.  The call only queues
 * launches on `stream`, with no host round trip; the launch geometry goes by n_symbols and the rooms
 * the caller names, never by a count on the device.  Every output element is written once, by one
 * lane, with no atomics on outputs.  *d_n_tokens is always the exact count for valid input.
 * *d_n_tokens > token_capacity: it is the capacity needed, the three token arrays are unspecified,
 * nothing was written outside [0 .. token_capacity), d_tok_first is complete and valid.  d_tok_id ==
 * NULL: count only (d_tok_first is still written).  *d_n > n_or_capacity (a scan that overflowed):
 * *d_n_tokens = 0 and nothing else is written.  In RUN and DROP mode the passes never read the text
 * and d_text may be NULL; in SYMBOL mode d_text may have any alignment that is a multiple of the
 * symbol size (the passes read only symbols of the buffer itself).  A contract violation -- a record
 * out of range, two records that overlap or are out of order, a record that crosses a text boundary,
 * a keyword_id >= n_keywords with d_tok_of given, offsets that decrease, do not begin with 0 or do not
 * end with n_symbols -- is handled as replace and grep handle theirs: a validation pass sees every
 * record, the offsets and the ids before any address is formed from them, acm_gpu_plan_status reports
 * ACM_GPU_E_INTERNAL, *d_n_tokens = 0, no other output is written and nothing is read or written out
 * of bounds.  The work is done in tiles of 8,192 symbols (ACM_GPU_TOKENS_TILE=<symbols> in the
 * environment sets another: a multiple of 64 from 64 to 16,384, read at every call -- by
 * acm_gpu_tokens_tmp_bytes too, whose answer is 16 bytes per tile: size the scratch under the setting
 * the call will see).
 *
 * acm_gpu_scan_tokens_device: with d_offsets == NULL acm_gpu_scan_select_device, with offsets (pos_base
 * must be 0 then) acm_gpu_scan_batch_device and acm_gpu_select_records_device over [0, n_symbols) -- a
 * batch's records never cross a text, so one selection serves all texts --, then the passes above,
 * all on `stream`; the selected records stay in d_records[0 .. *d_count).  The record capacity rule
 * is select's and the batch scan's: `capacity` must hold ALL matches of the buffer.  *d_count >
 * capacity afterwards: it is a capacity that suffices, and *d_n_tokens = 0.  With d_tok_of, n_keywords
 * must be at least acm_gpu_tally_keywords (plan), else ACM_GPU_E_ARG.  d_tmp (never NULL) must hold
 * acm_gpu_scan_tokens_tmp_bytes (plan, capacity, n_symbols, n_texts) bytes: the scans' and the
 * selection's scratch is reused, they have ended when the token passes begin.
 * acm_gpu_scan_tokens_host: the same from host memory, blocking.  The caller gives NO record capacity:
 * the call counts the matches first, as acm_gpu_scan_replace_host does.  ACM_GPU_E_OVERFLOW means only
 * "token_capacity is too small, *n_tokens suffices"; tok_first is valid then.  Offsets are checked on
 * the host (ACM_GPU_E_ARG).  tok_id == NULL counts: the two-call pattern is count, then fill.
 * n_selected (may be NULL) receives the number of selected matches.
 * acm_tokenize: the call on the machine itself, total over machines exactly as acm_replace is (same
 * three paths, same cached plan and acm_gpu_plan_update, acm_scan_path says which ran -- recorded on
 * success and on a token overflow): the GPU paths run acm_gpu_scan_tokens_host,
 * ACM_SCAN_PATH_CPU_LOOP runs the caller loop from the root at every offset into a record room the
 * call grows itself, then acm_select_records, then acm_tokens_records with the declared symbol size.
 * A tok_of with n_keywords below the machine's number of keywords is ACM_GPU_E_ARG on every path.  A
 * missing device stays an error, never a fallback. */
#define ACM_TOKENS_GAP_SYMBOL 0
#define ACM_TOKENS_GAP_RUN 1
#define ACM_TOKENS_GAP_DROP 2
int acm_tokens_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base,
                        const ACMRecord *records, uint64_t n,
                        const uint64_t *offsets /* NULL: one text */, uint64_t n_texts,
                        const uint32_t *tok_of /* NULL: the keyword ids */, uint64_t n_keywords,
                        uint32_t gap_base, uint32_t mode,
                        uint32_t *tok_id, uint64_t *tok_start, uint32_t *tok_len, uint64_t token_capacity,
                        uint64_t *n_tokens, uint64_t *tok_first);
size_t acm_gpu_tokens_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_symbols);
int acm_gpu_tokens_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                   const ACMRecord *d_sel, uint64_t n_or_capacity,
                                   const uint64_t *d_n /* device count, may be NULL: n is the count */,
                                   const uint64_t *d_offsets /* NULL: one text */, uint64_t n_texts,
                                   const uint32_t *d_tok_of /* NULL: the keyword ids */, uint64_t n_keywords,
                                   uint32_t gap_base, uint32_t mode,
                                   uint32_t *d_tok_id, uint64_t *d_tok_start, uint32_t *d_tok_len,
                                   uint64_t token_capacity, uint64_t *d_n_tokens, uint64_t *d_tok_first,
                                   void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_tokens_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_tokens_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                const uint64_t *d_offsets /* NULL: one text */, uint64_t n_texts,
                                ACMRecord *d_records, uint64_t capacity, uint64_t *d_count,
                                const uint32_t *d_tok_of, uint64_t n_keywords, uint32_t gap_base, uint32_t mode,
                                uint32_t *d_tok_id, uint64_t *d_tok_start, uint32_t *d_tok_len,
                                uint64_t token_capacity, uint64_t *d_n_tokens, uint64_t *d_tok_first,
                                void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_tokens_host (ACMPlan *plan, const void *text, uint64_t n_symbols,
                              const uint64_t *offsets /* NULL: one text */, uint64_t n_texts,
                              const uint32_t *tok_of, uint64_t n_keywords, uint32_t gap_base, uint32_t mode,
                              uint32_t *tok_id, uint64_t *tok_start, uint32_t *tok_len,
                              uint64_t token_capacity, uint64_t *n_tokens, uint64_t *tok_first,
                              uint64_t *n_selected);   /* blocking */
int acm_tokenize (ACMachine *machine, const void *text, uint64_t n_symbols,
                  const uint64_t *offsets /* NULL: one text */, uint64_t n_texts,
                  const uint32_t *tok_of, uint64_t n_keywords, uint32_t gap_base, uint32_t mode,
                  uint32_t *tok_id, uint64_t *tok_start, uint32_t *tok_len,
                  uint64_t token_capacity, uint64_t *n_tokens, uint64_t *tok_first, uint64_t *n_selected);

/* ------------------------------------------------------------------ grep over a batch
 * The reference's callers mostly hold many small texts -- log lines, packets, cells, the words of
 * examples/aho_corasick_generic_test.c:168-210, which restarts at the root for every word it reads,
 * the README's per-word loop -- and ask a dictionary what `grep -F -f` answers: which of my texts
 * contain a keyword, how many matches each has, and the matching (or the non-matching) texts
 * themselves, so that the next stage sees only those.  No record leaves the device and no record
 * capacity for the whole buffer has to be guessed: this is the batch counterpart of the tally.
 *
 * DEFINITION.  A batch is as in the batch scan: n_texts texts packed in one buffer, the same
 * offsets[0 .. n_texts] contract, empty texts allowed.  hits[t] is the number of records of text t
 * in acm_scan_batch's result, first[t + 1] - first[t]: the caller loop run from the root on every
 * text alone; a match that begins in an earlier text does not count.  KEPT is the ascending list of
 * the texts t with hits[t] > 0 when flags == ACM_GREP_MATCHING (0); with ACM_GREP_INVERT (1) it is
 * the texts with hits[t] == 0 (an empty text is never a hit, so INVERT keeps it).
 * kept[0 .. n_kept) holds their ids.  `total` is the sum of all hits[t], whatever the flags.
 * GATHER (optional: an output buffer is given): `out` is the symbols of the kept texts in order,
 * packed; out_offsets[0 .. n_kept] holds their offsets in `out`, out_offsets[0] = 0, and
 * out_symbols = out_offsets[n_kept].  The symbols are the caller's originals, bit for bit, in the
 * caller's symbol size -- never the class-mapped or interned copy a plan keeps for its scan
 * (acm_replace's rule).  kept/out_offsets/out are what the next acm_gpu_scan_batch_device,
 * acm_gpu_scan_replace_device or a tokeniser consumes directly on the device.
 *
 * acm_grep_gather: KEPT and GATHER from given hit counts, the plain sequential pass on the host, no
 * device; any sym_bytes > 0.  kept, out, out_offsets and out_symbols may be NULL (out NULL: nothing
 * is gathered, *out_symbols still says what it would take).  ACM_GPU_E_OVERFLOW with *out_symbols =
 * the length needed, and nothing written to `out`, when out_capacity (symbols) is too small: kept,
 * n_kept and out_offsets are written all the same.  ACM_GPU_E_ARG for offsets that do not begin with
 * 0 or that decrease, for flags above 1 and for n_texts >= 2^31.
 *
 * acm_gpu_grep_device: the same on the device (dev_grep.h), hits included.  Windows and record
 * capacity are acm_gpu_tally_device's: the buffer is cut into windows of window_symbols symbols (a
 * multiple of 16, greater than 0); every window starts from the root lmax - 1 symbols early, rounded
 * down to a 16-byte boundary of the text, and is scanned as acm_gpu_scan_device scans (any plan
 * kind, a pending delta included) into `capacity` records inside d_tmp; CAPACITY is per WINDOW,
 * greater than 0 and below 2^31, and capacity >= window_symbols x M (M as in the tally section)
 * cannot overflow.  There is no emit_from.  Outputs, all device memory, SET (not added to), valid
 * when `stream` has passed: d_hits (n_texts entries) and d_kept (room for n_texts ids) may be NULL,
 * d_out_offsets (room for n_texts + 1) may be NULL; *d_need = the largest record count of a window.
 *     some window found more than `capacity`:  *d_n_kept = *d_total = 0, *d_out_symbols = 0 when
 *         d_out is given, *d_need > capacity is a capacity that suffices for this window size;
 *         every other output is unspecified; nothing is written outside the buffers.
 * d_out NULL: no gather, and d_out_symbols must be NULL too (ACM_GPU_E_ARG when exactly one of the
 * two is NULL).  Gather overflow: *d_out_symbols > out_capacity afterwards is the capacity needed;
 * d_out is unspecified, nothing was written outside d_out[0 .. out_capacity), and d_hits, d_kept,
 * d_n_kept, d_total and d_out_offsets are complete and valid.  d_out must not overlap d_text
 * (ACM_GPU_E_ARG); both may have ANY byte alignment that is a multiple of the symbol size (the copy
 * loads whole aligned 16-byte words of the text: up to 15 bytes in front of and behind a text it
 * copies are read, never beyond the aligned word that holds a byte of that text) --
 * acm_gpu_replace_records_device's rule.  The output is built in tiles of 16,384 bytes
 * (ACM_GPU_GREP_TILE=<bytes> in the environment sets another: a multiple of 16 from 256 to 1 Mi,
 * read at every call).
 * n_texts >= 2^31 is ACM_GPU_E_ARG.  n_texts = 0 requires n_symbols = 0 and gives n_kept = 0.
 * d_offsets that break the contract (first not 0, last not n_symbols, decreasing) are handled as the
 * batch scan handles them: all counts are 0, no other output is written, acm_gpu_plan_status
 * reports ACM_GPU_E_INTERNAL, nothing is read or written out of bounds and no address is formed
 * from an offset before the check has seen it.  d_tmp must hold acm_gpu_grep_tmp_bytes (plan,
 * window_symbols, capacity, n_symbols, n_texts) bytes: 16 per record of capacity, 20 per text, 4 per
 * 4,096 symbols, 24 per 1,024 texts (0 for a capacity or an n_texts the call would refuse).  The
 * call only queues launches on `stream`, with no host round trip; one scan at a time per plan as
 * ever, and not while a stream (acm_gpu_stream_*) is open on it.
 * acm_gpu_grep_host: the same from host memory, blocking.  It picks the window and the capacity
 * exactly as acm_gpu_tally_host does (ACM_GPU_TALLY_CAPACITY included, repeated once with
 * window_symbols = capacity / M) and never reports a record overflow: ACM_GPU_E_OVERFLOW means only
 * "out_capacity is too small, *out_symbols suffices" -- hits, kept, n_kept, total and out_offsets
 * are valid then.  offsets[] is checked on the host (ACM_GPU_E_ARG; the last offset is the number of
 * symbols).  Every output pointer except n_kept may be NULL; out NULL: no gather, *out_symbols still
 * says what it would take.
 * acm_grep: the call on the machine itself, total over machines exactly as acm_tally is (same three
 * paths, same cached plan and acm_gpu_plan_update, acm_scan_path says which ran -- recorded on
 * success and on an output overflow): the GPU paths run acm_gpu_grep_host, ACM_SCAN_PATH_CPU_LOOP
 * runs the caller loop on the host from the root at every offset, counting the hits of every text,
 * then acm_grep_gather.  A missing device stays an error, never a fallback. */
#define ACM_GREP_MATCHING 0
#define ACM_GREP_INVERT 1
int acm_grep_gather (const void *text, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                     const uint64_t *hits, uint32_t flags, uint32_t *kept, uint64_t *n_kept,
                     void *out, uint64_t out_capacity, uint64_t *out_offsets, uint64_t *out_symbols);
size_t acm_gpu_grep_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity,
                               uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_grep_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols,
                         const uint64_t *d_offsets, uint64_t n_texts, uint32_t flags,
                         uint64_t window_symbols, uint64_t capacity,
                         uint64_t *d_hits /* n_texts, may be NULL */, uint32_t *d_kept /* n_texts, may be NULL */,
                         uint64_t *d_n_kept, uint64_t *d_total, uint64_t *d_need,
                         void *d_out /* may be NULL: no gather */, uint64_t out_capacity,
                         uint64_t *d_out_offsets /* n_texts + 1, may be NULL */,
                         uint64_t *d_out_symbols /* NULL iff d_out is */,
                         void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_grep_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                       uint32_t flags, uint64_t *hits, uint32_t *kept, uint64_t *n_kept, uint64_t *total,
                       void *out, uint64_t out_capacity, uint64_t *out_offsets,
                       uint64_t *out_symbols);   /* blocking */
int acm_grep (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
              uint32_t flags, uint64_t *hits, uint32_t *kept, uint64_t *n_kept, uint64_t *total,
              void *out, uint64_t out_capacity, uint64_t *out_offsets, uint64_t *out_symbols);

/* ------------------------------------------------------------------ per-text keyword counts of a batch
 * The tally says how often every keyword occurs in a buffer, grep how many matches every text of a
 * batch has.  This is their product: which keywords fired in which text, and how often -- the rule
 * set per packet of an IDS, the labels per log line, the bag-of-keywords row per document -- as a
 * text x keyword count matrix in CSR form, which is what a sparse-matrix consumer (torch's
 * sparse_csr_tensor among them) reads as it is.  No record leaves the device and no record capacity
 * for the whole buffer has to be guessed.
 *
 * DEFINITION.  A batch is as in the batch scan: n_texts texts packed in one buffer, the same
 * offsets[0 .. n_texts] contract, empty texts allowed.  C[t][k] is the number of records of text t
 * in acm_scan_batch's result whose keyword_id is k: the caller loop run from the root on every text
 * alone; a match that begins in an earlier text does not count.  The result is C in CSR form:
 * row_ptr[0 .. n_texts] (uint64_t, row_ptr[0] = 0), row t is the entries [row_ptr[t], row_ptr[t + 1])
 * of col[] (uint32_t keyword ids, strictly ascending within a row) and val[] (uint64_t counts, all
 * > 0); nnz = row_ptr[n_texts]; `total` is the sum of all val and equals grep's `total`.  Outputs
 * are SET, not added to.
 *
 * acm_tally_batch_records: C of a batch scan's records (any order within a text) and first[], the
 * plain sequential pass on the host, no device.  ACM_GPU_E_OVERFLOW with *nnz = the entries needed
 * when nnz_capacity is too small: col and val are untouched then, row_ptr is written all the same.
 * col and val may be NULL: the call only counts (row_ptr and *nnz) and returns ACM_GPU_OK.
 * ACM_GPU_E_ARG for a first[] that decreases or does not begin with 0, for a keyword_id >=
 * n_keywords and for n_texts >= 2^31.
 *
 * acm_gpu_tally_batch_device: the same on the device (dev_tally_batch.h).  Windows and the record
 * `capacity` per window are exactly acm_gpu_grep_device's (the same rules and the same *d_need, any
 * plan kind, a pending delta included, not while a stream is open).  The records of every window are
 * reduced to PARTIAL pairs (text, keyword, count) -- one block's share of a pair; a pair may have
 * several --, which are bucketed by text and merged.  pair_capacity (greater than 0, below 2^31) is
 * the room of d_col and d_val and also of the scratch area of the partial pairs, which are never
 * fewer than nnz and never more than the kept records (the records that count: `total`).  Outputs,
 * all device memory, valid when `stream` has passed; d_row_ptr has n_texts + 1 entries.
 *     no overflow:  every output is complete, *d_need <= capacity, and *d_need_pairs <= pair_capacity
 *         is the number of partial pairs this run made.
 *     some window found more than `capacity`:  *d_nnz = *d_total = 0, *d_need > capacity is a
 *         capacity that suffices for this window size; every other output is unspecified.
 *     more partial pairs than pair_capacity:  *d_nnz = *d_total = 0, *d_need_pairs > pair_capacity
 *         is the number of kept records of the call: a capacity that always suffices and that does
 *         not depend on the order in which the scan left its records (the number of partial pairs
 *         does); d_row_ptr, d_col and d_val are not written.
 * Nothing is ever written outside the buffers.  d_offsets that break the contract are handled as
 * grep handles them: *d_nnz = *d_total = *d_need_pairs = 0, d_row_ptr, d_col and d_val are not
 * written, acm_gpu_plan_status reports ACM_GPU_E_INTERNAL, and no address is formed from an offset
 * before the check has seen it.  A keyword_id that is no keyword of the plan (never expected) is not
 * counted and raises the same flag.  n_texts >= 2^31 is ACM_GPU_E_ARG; n_texts = 0 requires
 * n_symbols = 0 and gives row_ptr[0] = 0, nnz = 0.  d_tmp must hold acm_gpu_tally_batch_tmp_bytes
 * (plan, window_symbols, capacity, pair_capacity, n_symbols, n_texts) bytes: 16 per record of
 * capacity, 28 per pair of pair_capacity, 28 per text, 4 per 4,096 symbols, 64 per keyword (0 for
 * arguments the call would refuse).  A row of more than 2,048 partial pairs is merged by a slow
 * form that is always correct.  In the environment, read at every call (tests, experiments):
 * ACM_GPU_TALLY_BATCH_SLOTS=<a power of two from 8 to 4,096> is the size of a block's table of
 * pairs, ACM_GPU_TALLY_BATCH_ROW=<1 to 2,048> the widest row of the fast form.  The call only
 * queues launches on `stream`, with no host round trip.
 * acm_gpu_tally_batch_host: the same from host memory, blocking.  It picks the window and the record
 * capacity exactly as acm_gpu_tally_host does (ACM_GPU_TALLY_CAPACITY included, repeated once with
 * window_symbols = capacity / M), picks a pair room by itself and repeats once with *d_need_pairs
 * when that was too small.  ACM_GPU_E_OVERFLOW means only "nnz_capacity is too small, *nnz
 * suffices": row_ptr, total and nnz are valid then, col and val untouched.  col and val may be
 * NULL: the call only counts.  offsets[] is checked on the host (ACM_GPU_E_ARG).
 * acm_tally_batch: the call on the machine itself, total over machines exactly as acm_grep is (same
 * three paths, same cached plan and acm_gpu_plan_update, acm_scan_path says which ran -- recorded on
 * success and on an output overflow): the GPU paths run acm_gpu_tally_batch_host,
 * ACM_SCAN_PATH_CPU_LOOP runs the caller loop on the host from the root at every offset into a
 * record room the call grows itself, then acm_tally_batch_records.  A missing device stays an
 * error, never a fallback. */
int acm_tally_batch_records (const ACMRecord *records, const uint64_t *first, uint64_t n_texts,
                             uint64_t n_keywords, uint64_t *row_ptr, uint32_t *col, uint64_t *val,
                             uint64_t nnz_capacity, uint64_t *nnz);
size_t acm_gpu_tally_batch_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity,
                                      uint64_t pair_capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_tally_batch_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols,
                                const uint64_t *d_offsets, uint64_t n_texts,
                                uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity,
                                uint64_t *d_row_ptr /* n_texts + 1 */, uint32_t *d_col, uint64_t *d_val,
                                uint64_t *d_nnz, uint64_t *d_total, uint64_t *d_need, uint64_t *d_need_pairs,
                                void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_tally_batch_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                              uint64_t *row_ptr, uint32_t *col, uint64_t *val, uint64_t nnz_capacity,
                              uint64_t *nnz, uint64_t *total);   /* blocking */
int acm_tally_batch (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
                     uint64_t *row_ptr, uint32_t *col, uint64_t *val, uint64_t nnz_capacity,
                     uint64_t *nnz, uint64_t *total);

/* ------------------------------------------------------------------ keyword rules per text
 * The count matrix above says which keywords a text holds.  A signature of an IDS, a YARA rule or a
 * log classifier is a COMBINATION of keywords: "A and B", "A but not B", "any two of these five",
 * "A at least three times".  These calls evaluate a set of such rules on every text of a batch, on
 * the device, behind the tally: which rules fired in which text, so that the stage that decides
 * which texts the next stage sees needs no copy of the matrix to the host.
 *
 * DEFINITION.  C[t][k] is acm_tally_batch's matrix; the batch contract, the offsets contract and
 * empty texts are the same as there.
 *   A TERM is (keyword_id, lo, hi), three uint32_t (ACMRuleTerm).  It HOLDS for text t iff
 *     lo <= C[t][keyword_id] <= hi; hi = ACM_RULE_NO_MAX (0xFFFFFFFF) is no upper bound: a count
 *     above 2^32 still holds such a term.  (k, 1, NO_MAX) is "k present", (k, 0, 0) "k absent",
 *     (k, 3, NO_MAX) "k at least three times", (k, 2, 3) an interval; (k, 0, NO_MAX) always holds and
 *     is allowed.  lo > hi is ACM_GPU_E_ARG.
 *   A RULE r is the terms [rule_ptr[r], rule_ptr[r + 1]) of terms[] (rule_ptr: uint64_t, n_rules + 1
 *     entries) and need[r] (uint32_t).  It FIRES for t iff at least need[r] of its terms hold:
 *     need = the number of terms is AND, need = 1 is OR, anything between is "m of n".  One keyword
 *     may occur in several terms of one rule (two disjoint intervals).  ACM_GPU_E_ARG: a rule without
 *     terms, need[r] = 0, need[r] above the rule's number of terms, a rule_ptr that decreases or does
 *     not begin with 0, a keyword_id >= n_keywords, n_rules >= 2^31.
 *   The RESULT is the text x rule boolean matrix in CSR form: fired_ptr[0 .. n_texts] (uint64_t,
 *     fired_ptr[0] = 0), row t is the rule ids fired[fired_ptr[t] .. fired_ptr[t + 1]) (uint32_t,
 *     strictly ascending); n_fired = fired_ptr[n_texts].  Outputs are SET, not added to.
 * A rule whose terms that hold at count 0 already reach `need` fires on a text with no keyword at
 * all, an empty text among them: "absent he" fires on "".
 * Keyword ids are first-insertion ranks, so a rule set stays valid when the dictionary grows
 * (acm_gpu_plan_update); keywords added later occur in no rule.
 *
 * acm_rules_check: the argument checks above, no device; every other entry point runs it.
 * acm_rules_matrix: the plain sequential evaluation of a given count matrix (row_ptr, col, val as
 * acm_tally_batch gives them) on the host.  ACM_GPU_E_OVERFLOW with *n_fired = the entries needed
 * when fired_capacity is too small: `fired` is untouched then, fired_ptr is written all the same.
 * `fired` may be NULL: the call only counts and returns ACM_GPU_OK.  A row_ptr that decreases or
 * does not begin with 0 and a col >= n_keywords are ACM_GPU_E_ARG (acm_tally_batch_records' rule).
 *
 * acm_gpu_rules_create: a rule set is compiled once, on the host, into an index inverted by keyword
 * and uploaded to the plan's device: post_ptr[n_keywords + 1], the postings (rule, lo, hi) of every
 * keyword (a term that holds at every count has none: it only counts into base), base[r] = the
 * number of r's terms that hold at count 0, need[r], and the ascending list of the ALWAYS-RULES,
 * those with base[r] >= need[r].  n_keywords is acm_gpu_tally_keywords (plan) at creation; the set
 * belongs to the plan's device and serves that plan, also after acm_gpu_plan_update.  2^31 terms
 * or more are ACM_GPU_E_ARG.  acm_gpu_rules_info waits for the device and reports the sizes
 * and how many texts the set's evaluations have sent through the fast and through the wide form
 * since creation (below).
 *
 * acm_gpu_rules_matrix_device: the evaluation of ANY count matrix that lies on the device,
 * acm_gpu_tally_batch_device's or a caller's own (rows ascending by keyword id without repeats).
 * One wave takes one text (dev_rules.h): every posting of every keyword of the row whose holding
 * differs from holding at count 0 is an item (rule, +1 / -1); the items are sorted by rule in the
 * wave's LDS and summed per rule; rule r fires iff base[r] + sum >= need[r]; the sorted touched
 * rules are merged with the always-list.  A text with more items than the fast form has room for
 * is taken by a block that sorts in scratch (the wide form: slower, always correct).  A count pass
 * fills d_fired_ptr, a fill pass d_fired: work per text goes by the postings of the row's keywords
 * and the always-list, no memory is sized n_texts x n_rules.  Outputs, all device memory, valid when
 * `stream` has passed:
 *     *d_n_fired <= fired_capacity:  every output is complete.
 *     *d_n_fired > fired_capacity:  it is the capacity needed; d_fired_ptr is complete and valid,
 *         d_fired unspecified; nothing is written outside d_fired[0 .. fired_capacity).
 * d_fired may be NULL with fired_capacity = 0: the call only counts.  A d_row_ptr that breaks the
 * contract is handled as tally_batch handles offsets: *d_n_fired = 0, nothing else is written,
 * acm_gpu_plan_status reports ACM_GPU_E_INTERNAL, and no address is formed from a row pointer before
 * the check has seen it.  A d_col entry >= the rule set's n_keywords is skipped, not flagged: after
 * acm_gpu_plan_update the matrix may hold newer keywords.  n_texts >= 2^31 is ACM_GPU_E_ARG;
 * n_texts = 0 gives fired_ptr[0] = 0 and n_fired = 0.  d_tmp must hold acm_gpu_rules_matrix_tmp_bytes
 * (plan, rules, n_texts) bytes: 20 per text and 96 per posting of the set.  In the environment, read
 * at every call (tests, experiments): ACM_GPU_RULES_ITEMS=<1 to 4,096> is the widest text, in items,
 * that takes the fast form (1,024 when absent).  The call only queues launches on `stream`, with no
 * host round trip.
 * acm_gpu_rules_device: acm_gpu_tally_batch_device into a matrix inside d_tmp, then the evaluation,
 * queued in one call (any plan kind, a pending delta included, not while a stream is open).
 * Windows, `capacity`, pair_capacity, *d_total, *d_need and *d_need_pairs are exactly tally_batch's;
 * when a window or the pairs overflowed, or d_offsets break the contract, *d_n_fired = 0 and
 * d_fired_ptr and d_fired are not written.  d_tmp must hold acm_gpu_rules_tmp_bytes (plan, rules,
 * window_symbols, capacity, pair_capacity, n_symbols, n_texts) bytes.
 * acm_gpu_rules_host: the same from host memory, blocking, with the rule arrays: it creates and
 * destroys the set itself and picks and repeats the rooms exactly as acm_gpu_tally_batch_host does.
 * ACM_GPU_E_OVERFLOW means only "fired_capacity is too small, *n_fired suffices": fired_ptr, total
 * and n_fired are valid then, `fired` untouched.  `fired` may be NULL: the call only counts.
 * acm_rules: the call on the machine itself, total over machines exactly as acm_tally_batch is
 * (same three paths, same cached plan, acm_scan_path recorded on success and on an output overflow):
 * the GPU paths run acm_gpu_rules_host, ACM_SCAN_PATH_CPU_LOOP runs acm_tally_batch's host loop
 * into a room the call grows itself, then acm_rules_matrix.  A missing device stays an error, never
 * a fallback.
 * Out of scope: positional rules (distance, order, offset), regular expressions, per-rule hit
 * counts on the device (a bincount of fired[]), flows, several GPUs.  Weighted sums of the counts,
 * thresholds on them, the best class of a text and the best texts of a class are acm_score.h's. */
#define ACM_RULE_NO_MAX 0xFFFFFFFFu
typedef struct {
  uint32_t keyword_id, lo, hi;
} ACMRuleTerm;
typedef struct ACMRules ACMRules;
typedef struct {
  uint64_t rules, terms, always_rules, postings;
  uint64_t fast_texts, wide_texts; /* texts evaluated by either form since creation (count passes) */
} ACMRulesInfo;
int acm_rules_check (const ACMRuleTerm *terms, const uint64_t *rule_ptr, const uint32_t *need,
                     uint64_t n_rules, uint64_t n_keywords);
int acm_rules_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts,
                      uint64_t n_keywords, const ACMRuleTerm *terms, const uint64_t *rule_ptr,
                      const uint32_t *need, uint64_t n_rules, uint64_t *fired_ptr /* n_texts + 1 */,
                      uint32_t *fired, uint64_t fired_capacity, uint64_t *n_fired);
int acm_gpu_rules_create (ACMPlan *plan, const ACMRuleTerm *terms, const uint64_t *rule_ptr,
                          const uint32_t *need, uint64_t n_rules, ACMRules **out);
void acm_gpu_rules_destroy (ACMRules *rules);
int acm_gpu_rules_info (const ACMRules *rules, ACMRulesInfo *info);
size_t acm_gpu_rules_matrix_tmp_bytes (const ACMPlan *plan, const ACMRules *rules, uint64_t n_texts);
int acm_gpu_rules_matrix_device (ACMPlan *plan, const ACMRules *rules, const uint64_t *d_row_ptr,
                                 const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts,
                                 uint64_t *d_fired_ptr /* n_texts + 1 */, uint32_t *d_fired,
                                 uint64_t fired_capacity, uint64_t *d_n_fired, void *d_tmp,
                                 size_t tmp_bytes, void *stream);
size_t acm_gpu_rules_tmp_bytes (const ACMPlan *plan, const ACMRules *rules, uint64_t window_symbols,
                                uint64_t capacity, uint64_t pair_capacity, uint64_t n_symbols,
                                uint64_t n_texts);
int acm_gpu_rules_device (ACMPlan *plan, const ACMRules *rules, const void *d_text, uint64_t n_symbols,
                          const uint64_t *d_offsets, uint64_t n_texts, uint64_t window_symbols,
                          uint64_t capacity, uint64_t pair_capacity, uint64_t *d_fired_ptr /* n_texts + 1 */,
                          uint32_t *d_fired, uint64_t fired_capacity, uint64_t *d_n_fired,
                          uint64_t *d_total, uint64_t *d_need, uint64_t *d_need_pairs, void *d_tmp,
                          size_t tmp_bytes, void *stream);
int acm_gpu_rules_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                        const ACMRuleTerm *terms, const uint64_t *rule_ptr, const uint32_t *need,
                        uint64_t n_rules, uint64_t *fired_ptr, uint32_t *fired, uint64_t fired_capacity,
                        uint64_t *n_fired, uint64_t *total);   /* blocking */
int acm_rules (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
               const ACMRuleTerm *terms, const uint64_t *rule_ptr, const uint32_t *need, uint64_t n_rules,
               uint64_t *fired_ptr, uint32_t *fired, uint64_t fired_capacity, uint64_t *n_fired,
               uint64_t *total);

/* ------------------------------------------------------------------ a buffer cut into texts: the batch calls' front end
 * Every batch call above takes offsets[] as given.  A caller with a file or a capture holds ONE
 * buffer with delimiters in it -- log lines, cells, the words that
 * examples/aho_corasick_generic_test.c:168-210 reads one by one -- and these calls make the offsets
 * from it, on the device, so that the text never has to visit the host for it.
 *
 * DEFINITION.  SPLIT (text[0 .. n), delims[0 .. d), flags); all symbols have the caller's symbol
 * size; 1 <= d <= 16 (ACM_SPLIT_MAX_DELIMS).
 *   is_delim (i): text[i] equals one of delims[] BIT FOR BIT, in the caller's symbols -- never in the
 *     class-mapped or interned copy a plan keeps for its scan (acm_replace's rule): under a
 *     case-folding comparator and the delimiter "x", "X" is no delimiter.
 *   ACM_SPLIT_EVERY (0): there is a cut behind every i with is_delim (i).  These are lines:
 *     "a\n\nb" is the three texts "a\n", "\n", "b".
 *   ACM_SPLIT_RUNS (1): there is a cut behind i when is_delim (i) and (i + 1 == n or not
 *     is_delim (i + 1)).  These are words: a text is a word with the whole run of delimiters that
 *     follows it; a run at the very front of the buffer is a text of its own.
 *   In both modes there is a cut behind n - 1 when n > 0: an unterminated last line is a text.
 *   offsets = [0] ++ [i + 1 for every cut, ascending]; n_texts = the number of cuts; n = 0 gives
 *   n_texts = 0 and offsets = [0].
 * Offsets ascend strictly, offsets[0] = 0 and offsets[n_texts] = n: exactly the batch contract (no
 * text is empty), so the result feeds every acm_gpu_*_batch / flows / grep / tally_batch call as it
 * is.  The delimiter is the LAST symbol(s) of the text it ends: the gathered output of a grep
 * reproduces the kept lines with their newlines, as `grep` prints them.  A keyword that contains a
 * delimiter can therefore match only at the end of a text (under RUNS, and for a keyword of
 * several delimiters, only in the run that ends one).
 *
 * acm_split_offsets: the plain sequential pass on the host, no device; any sym_bytes > 0 (memcmp).
 * offsets (room for capacity + 1) may be NULL: the call only counts and ignores capacity.
 * ACM_GPU_E_OVERFLOW with *n_texts = the count needed, and nothing written to offsets, when
 * capacity is too small.  ACM_GPU_E_ARG for n_delims of 0 or above 16 and for flags above 1.
 *
 * acm_gpu_split_device: the same on the device (dev_split.h).  The symbol size is the plan's caller
 * symbol size (1, 2, 4 or 8); the plan is used for nothing but its device, that size and its grid
 * cap, so a plan with a pending delta, a class plan and an interned 8-byte plan behave alike, and no
 * contract can be broken by data: acm_gpu_plan_status is not involved.  `delims` is HOST memory,
 * n_delims symbols; they travel as kernel arguments, nothing is copied and delims may be freed on
 * return.  Outputs, device memory, valid when `stream` has passed: *d_n_texts is always the exact
 * count; d_offsets[0 .. *d_n_texts] when *d_n_texts <= capacity.  *d_n_texts > capacity: it is the
 * capacity needed, d_offsets[0 .. capacity] is unspecified and nothing was written outside it.
 * d_offsets NULL: the call only counts and ignores capacity.  ACM_GPU_E_ARG: capacity >= 2^31 with
 * d_offsets given (the batch calls refuse such an n_texts anyway), n_delims of 0 or above 16, flags
 * above 1, a d_text that is no multiple of the symbol size, a tmp_bytes that is too small.  d_text
 * may have ANY alignment that is a multiple of the symbol size: the kernels load whole aligned
 * 16-byte words (replace's and grep's rule: up to 15 bytes in front of and behind the buffer are
 * read, never beyond the aligned word that holds a byte of it), and a symbol outside [0, n) never
 * counts, whatever its value.  Two passes over tiles of 16,384 bytes of the text
 * (ACM_GPU_SPLIT_TILE=<bytes> in the environment sets another: a multiple of 16 from 256 to 1 Mi,
 * read at every call) with a prefix sum over the tiles' counts between them.  d_tmp must hold
 * acm_gpu_split_tmp_bytes (plan, n_symbols) bytes -- 16 per tile, for the tile size in force -- (0
 * for a buffer the call would refuse).  The call only queues launches on `stream`, with no host
 * round trip.
 * acm_gpu_split_host: the same from host memory, blocking.  ACM_GPU_E_OVERFLOW with *n_texts = the
 * count needed when capacity is too small.
 *
 * acm_gpu_grep_lines_host: `grep -F -f keywords file` on a raw buffer in host memory, blocking.  The
 * text is uploaded once and split on the device -- a count run, ONE host round trip for n_texts,
 * which sizes the per-text buffers, then the run that writes the offsets --, then grep runs exactly
 * as acm_gpu_grep_host runs it (same window and capacity choice, ACM_GPU_TALLY_CAPACITY, the one
 * repeat).  *n_texts and *n_kept are required.  offsets (texts_capacity + 1 entries), hits, kept
 * (texts_capacity each) and out_offsets (texts_capacity + 1) are optional.  ACM_GPU_E_OVERFLOW has
 * two meanings, told apart by the caller: *n_texts > texts_capacity while a per-text array was
 * asked for -- only *n_texts is valid, nothing else was written --; otherwise *out_symbols >
 * out_capacity -- everything but `out` is valid, as in acm_gpu_grep_host.  With all four per-text
 * pointers NULL there is no first kind.  A buffer of 2^31 texts or more is ACM_GPU_E_ARG
 * (*n_texts says how many).
 * acm_grep_lines: the call on the machine itself, total over machines exactly as acm_grep is (same
 * three paths, acm_scan_path recorded on success and on either overflow): the GPU paths run
 * acm_gpu_grep_lines_host, ACM_SCAN_PATH_CPU_LOOP runs acm_split_offsets with the declared symbol
 * size, then the host loop acm_grep uses, then acm_grep_gather.  A missing device stays an error. */
#define ACM_SPLIT_EVERY 0
#define ACM_SPLIT_RUNS 1
#define ACM_SPLIT_MAX_DELIMS 16
int acm_split_offsets (const void *text, uint64_t n_symbols, uint32_t sym_bytes,
                       const void *delims, uint32_t n_delims, uint32_t flags,
                       uint64_t *offsets /* capacity + 1, may be NULL: count only */, uint64_t capacity,
                       uint64_t *n_texts);
size_t acm_gpu_split_tmp_bytes (const ACMPlan *plan, uint64_t n_symbols);
int acm_gpu_split_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols,
                          const void *delims /* HOST memory, n_delims symbols */, uint32_t n_delims, uint32_t flags,
                          uint64_t *d_offsets /* capacity + 1, may be NULL: count only */, uint64_t capacity,
                          uint64_t *d_n_texts, void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_split_host (ACMPlan *plan, const void *text, uint64_t n_symbols, const void *delims, uint32_t n_delims,
                        uint32_t flags, uint64_t *offsets, uint64_t capacity, uint64_t *n_texts);   /* blocking */
int acm_gpu_grep_lines_host (ACMPlan *plan, const void *text, uint64_t n_symbols,
                             const void *delims, uint32_t n_delims, uint32_t split_flags, uint32_t grep_flags,
                             uint64_t *n_texts, uint64_t *n_kept, uint64_t *total,
                             void *out, uint64_t out_capacity, uint64_t *out_symbols,
                             uint64_t texts_capacity, uint64_t *offsets, uint64_t *hits, uint32_t *kept,
                             uint64_t *out_offsets);   /* blocking */
int acm_grep_lines (ACMachine *machine, const void *text, uint64_t n_symbols,
                    const void *delims, uint32_t n_delims, uint32_t split_flags, uint32_t grep_flags,
                    uint64_t *n_texts, uint64_t *n_kept, uint64_t *total,
                    void *out, uint64_t out_capacity, uint64_t *out_symbols,
                    uint64_t texts_capacity, uint64_t *offsets, uint64_t *hits, uint32_t *kept,
                    uint64_t *out_offsets);

/* ------------------------------------------------------------------ whole-word matches
 * Every consumer above acts on the raw match set: with {he, she, his, hers} a replacer built on
 * acm_replace rewrites the "he" inside "the", "other" and "where".  `grep -w` and keyword
 * extraction exist to prevent that.  WORDS is the record filter that looks at the two symbols next
 * to a match.  It runs in front of SELECT -- the leftmost-longest tiling is taken among the
 * whole-word matches -- and has acm_gpu_select_records_device's calling shape, so it composes with
 * the select, replace and tokens passes with no change to any of them.
 *
 * DEFINITION.  The word set is ranges[0 .. 2 * n_ranges) in the caller's symbol size: pair j is the
 * inclusive range [lo_j, hi_j], symbols compared as unsigned little-endian integers of sym_bytes
 * bytes; 1 <= n_ranges <= 16 (ACM_WORDS_MAX_RANGES); a pair with lo > hi is ACM_GPU_E_ARG.
 * is_word (x) holds when x lies in some range.  It is tested on the caller's ORIGINAL symbols, bit
 * for bit -- never on the class-mapped or interned copy a plan keeps for its scan (acm_replace's
 * rule): under a case-folding comparator and the range a-z, "A" is no word symbol.  The usual ASCII
 * set is the four ranges  0-9, A-Z, _, a-z  = { '0','9', 'A','Z', '_','_', 'a','z' }; callers with
 * UTF-8 byte text add [0x80, 0xFF].
 * Texts: offsets[0 .. n_texts] follows the batch contract (first 0, last n_symbols, never
 * decreasing, empty texts allowed); offsets == NULL means that the buffer is one text.
 * WORDS (R, text, offsets, ranges, flags).  For a record r let s = end_pos + 1 - length - pos_base,
 * e = end_pos - pos_base and t the text with offsets[t] <= s < offsets[t + 1].  Then
 *   left_ok (r):  s == offsets[t] or not is_word (text[s - 1]);
 *   right_ok (r): e + 1 == offsets[t + 1] or not is_word (text[e + 1]);
 *   ACM_WORDS_LEFT (1) keeps r when left_ok holds (matches that begin a word), ACM_WORDS_RIGHT (2)
 *   when right_ok holds (matches that end a word), ACM_WORDS_BOTH (3) when both hold: `grep -w`'s
 *   test.  flags of 0 or above 3 is ACM_GPU_E_ARG.
 * The match's own symbols are not looked at: a keyword "e.g." or "New York" is whole-word when its
 * neighbours are no word symbols.  A symbol outside its text never counts, whatever its value: the
 * one in front of offsets[t], the one behind offsets[t + 1] - 1, anything outside [0, n_symbols);
 * such a symbol is never loaded.  With offsets given, a record with e >= offsets[t + 1] (a match
 * that spans a cut) is dropped silently, so WORDS of the ordered scan of the packed buffer equals
 * WORDS of acm_scan_batch's records.  The output is the kept records in the order of the input
 * (stable); the input order is arbitrary, so the filter also runs on acm_gpu_scan_device's
 * unordered records, in front of an order pass that then has less to do.
 *
 * acm_words_records: the plain sequential pass on the host, no device, in place in the front of
 * the array; sym_bytes 1, 2, 4 or 8 (another size is ACM_GPU_E_ARG).  Offsets that break the batch
 * contract, a record outside [pos_base, pos_base + n_symbols) (its end or its start) or of length
 * 0: ACM_GPU_E_ARG, nothing modified.
 *
 * acm_gpu_words_records_device: the same on the device (dev_words.h), acm_gpu_select_records_device's
 * shape: d_n NULL -- n_or_capacity is the number of records; d_n given -- *d_n is, and n_or_capacity
 * the room of d_records and d_out (below 2^31).  *d_n > n_or_capacity (a scan that overflowed):
 * nothing is kept and *d_count = *d_n.  The call only queues launches on `stream`, with no host
 * round trip.  The plan is used for its device, its caller symbol size and its grid cap only: class
 * plans, interned 8-byte plans and plans with a pending delta behave alike.  `ranges` is HOST
 * memory, 2 * n_ranges symbols; they travel as kernel arguments and may be freed on return.
 * d_count may be d_n; d_out must not overlap d_records (ACM_GPU_E_ARG).  d_text may have any
 * alignment that is a multiple of the symbol size (the neighbours are loaded as single naturally
 * aligned symbols).  Two passes over tiles of 4,096 records (ACM_GPU_WORDS_TILE=<records> in the
 * environment sets another: a multiple of 64 from 64 to 1 Mi, read at every call) with a prefix sum
 * over the tiles' counts between them; d_tmp must hold acm_gpu_words_tmp_bytes (plan,
 * n_or_capacity, n_texts) bytes (0 for a call that would be refused).  A record that breaks the
 * contract (a position outside [pos_base, pos_base + n_symbols), a start below pos_base, a length
 * of 0) is dropped, nothing is read or written out of bounds and acm_gpu_plan_status reports
 * ACM_GPU_E_INTERNAL (select's rule).  d_offsets that break the batch contract are handled as the
 * batch scan handles them: *d_count = 0, no other output, status ACM_GPU_E_INTERNAL; no address is
 * formed from an offset before the check has seen it.
 *
 * acm_gpu_scan_words_device: the filter applied to acm_gpu_scan_ordered_device's records with
 * emit_from = 0, in canonical order.  capacity must hold ALL matches (select's rule): *d_count <=
 * capacity -- the count is exact and the records are complete; *d_count > capacity -- it is the
 * scan's count and the records are unspecified.
 * acm_gpu_scan_words_host: the same from host memory, blocking.  ACM_GPU_E_OVERFLOW with *n_found
 * = a capacity that suffices.  Offsets that break the batch contract are ACM_GPU_E_ARG.
 * acm_scan_words: the call on the machine itself, for one text, total over machines exactly as
 * acm_select is (same three paths, same cached plan, acm_scan_path recorded on success and on
 * overflow): ACM_SCAN_PATH_CPU_LOOP runs the caller loop and then acm_words_records.  Batch callers
 * filter acm_scan_batch's records with acm_words_records or the device call.  A missing device
 * stays an error.
 *
 * Out of scope: whole-word flags inside acm_grep, acm_tally, acm_tally_batch and acm_tokenize (their
 * signatures do not change); several GPUs, streams and flows; Unicode property tables beyond 16
 * ranges. */
#define ACM_WORDS_LEFT 1
#define ACM_WORDS_RIGHT 2
#define ACM_WORDS_BOTH 3
#define ACM_WORDS_MAX_RANGES 16
int acm_words_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base,
                       const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                       const void *ranges, uint32_t n_ranges, uint32_t flags,
                       ACMRecord *records, uint64_t n, uint64_t *n_kept);   /* in place, front of the array */
size_t acm_gpu_words_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_texts);
int acm_gpu_words_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                  const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                  const void *ranges /* HOST memory, 2 * n_ranges symbols */, uint32_t n_ranges, uint32_t flags,
                                  const ACMRecord *d_records, uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                  ACMRecord *d_out, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_words_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_words_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                               const uint64_t *d_offsets, uint64_t n_texts,
                               const void *ranges, uint32_t n_ranges, uint32_t flags,
                               ACMRecord *d_records, uint64_t capacity, uint64_t *d_count,
                               void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_words_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                             const uint64_t *offsets, uint64_t n_texts,
                             const void *ranges, uint32_t n_ranges, uint32_t flags,
                             ACMRecord *records, uint64_t capacity, uint64_t *n_found);   /* blocking */
int acm_scan_words (ACMachine *machine, const void *text, uint64_t n_symbols,
                    const void *ranges, uint32_t n_ranges, uint32_t flags,
                    ACMRecord *records, uint64_t capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ match contexts: the text around the matches
 * Every consumer above answers with numbers.  What people do with a match list is look at the text
 * around it: `grep -C 2` prints the hit lines with their neighbours, a concordance wants 40 symbols
 * on both sides of every hit, a log triage tool the matching packet with the two in front of it, a
 * reviewer of acm_scan_approx's, acm_scan_chains' or acm_scan_templates' hits the stretch each one
 * lies in.  CONTEXT turns records into windows, merges them, and copies them out into one packed
 * buffer with the index a highlighter needs -- on the device, so that the text need not come back
 * for it.  It takes ANY record array of the ACMRecord layout: the record sets of acm_scan_words,
 * acm_select, acm_scan_patterns, acm_scan_approx, acm_scan_chains and acm_scan_templates go through
 * it unchanged.
 *
 * DEFINITION.  Inputs: text[0 .. n_symbols) in the caller's symbols, sym_bytes 1, 2, 4 or 8, copied
 * bit for bit -- never the class-mapped or interned copy a plan keeps for its scan (acm_replace's
 * rule); offsets[0 .. n_texts] under the batch contract, or NULL: one text; records r_0 .. r_{m-1}
 * with pos_base, as in WORDS; `before` and `after`; flags = the unit in bit 0, ACM_CONTEXT_SYMBOLS
 * (0) or ACM_CONTEXT_TEXTS (1), and the mode in bit 1, ACM_CONTEXT_EACH (0) or ACM_CONTEXT_MERGE
 * (2).  Flags above 3, and TEXTS with offsets NULL, are ACM_GPU_E_ARG.
 * For a record r let s = end_pos + 1 - length - pos_base, e = end_pos - pos_base and t the text with
 * offsets[t] <= s < offsets[t + 1].  A record with e >= offsets[t + 1] spans a cut and is
 * WINDOWLESS (WORDS' rule: the ordered scan of a packed buffer can be fed in as it is).  The window
 * W (r) = [lo, hi), all arithmetic saturating (before = 2^32 - 1 is legal):
 *   SYMBOLS: lo = max (offsets[t], s - before), hi = min (offsets[t + 1], e + 1 + after); with
 *            offsets NULL offsets[t] is 0 and offsets[t + 1] is n_symbols;
 *   TEXTS:   lo = offsets[max (0, t - before)], hi = offsets[min (n_texts, t + 1 + after)]: the
 *            match's text with `before` texts in front and `after` behind, `grep -B` and `grep -A`.
 * EACH: snippet j is W (r_j), j = 0 .. m - 1, in the order of the input (any order), n_snippets = m;
 * a windowless record gives an empty snippet, at its own start s.
 * MERGE: let C be the union of all windows.  The snippets are the maximal runs of consecutive
 * positions in C, ascending.  Under SYMBOLS a run is also cut at every text boundary inside it: two
 * windows that touch across offsets[t] stay two snippets, two that touch inside a text are one.
 * Under TEXTS runs are not cut, a snippet is a run of whole texts: how `grep -C` joins overlapping
 * and adjacent context groups.  MERGE requires end_pos never to decrease over the records;
 * canonical order satisfies it.
 * Outputs: n_snippets; snip_lo[j], the buffer index of the snippet's first symbol, without
 * pos_base; out_offsets[0 .. n_snippets], out_offsets[0] = 0; out = the concatenation of
 * text[snip_lo[j] .. snip_lo[j] + len_j); out_symbols = out_offsets[n_snippets]; optional
 * snip_text[j] (uint32_t), the text that holds the symbol snip_lo[j] (0 without offsets; behind an
 * empty text under TEXTS it is the first text of the run that has a symbol); optional rec_snip[i]
 * (uint32_t), the snippet record i lies in, 0xFFFFFFFF (ACM_CONTEXT_NONE) when windowless; optional
 * rec_at[i] (int64_t), the index in `out` of the match's first symbol, out_offsets[rec_snip[i]] +
 * s_i - snip_lo[rec_snip[i]], -1 when windowless: the offset map a highlighter uses, the
 * counterpart of replace's out_start.  n_snippets <= m: the per-snippet arrays are sized by the
 * record room (out_offsets one more).
 *
 * acm_context_records: the plain sequential pass on the host, no device.  n_snippets and out_symbols
 * are required, every array may be NULL.  `out` NULL: nothing is gathered, *out_symbols still says
 * what it takes.  ACM_GPU_E_OVERFLOW when out_capacity (symbols) is too small: *out_symbols is the
 * length needed, nothing is written to `out`, every index array is valid (acm_grep_gather's rule).
 * ACM_GPU_E_ARG: offsets that break the batch contract, a record outside [pos_base, pos_base +
 * n_symbols) (its end or its start) or of length 0, MERGE over records whose end_pos decreases, m
 * or n_texts of 2^31 or more; nothing is written then.
 *
 * acm_gpu_context_records_device: the same on the device (dev_context.h).  The text, offsets,
 * records, d_n and n_or_capacity arguments are acm_gpu_words_records_device's (d_n NULL:
 * n_or_capacity is the number of records; else *d_n is, and n_or_capacity the room, below 2^31), the
 * output arguments acm_gpu_replace_records_device's.  d_n_snippets, d_out_symbols (8 bytes each),
 * d_snip_lo (n_or_capacity entries) and d_out_offsets (n_or_capacity + 1) are required; d_snip_text,
 * d_rec_snip and d_rec_at (n_or_capacity each) may be NULL.  The call only queues launches on
 * `stream`, with no host round trip; the plan is used for its device, its caller symbol size and
 * its grid cap only.  d_out NULL: no gather, *d_out_symbols is still written.  *d_out_symbols >
 * out_capacity afterwards: it is the capacity needed, d_out is unspecified, nothing was written
 * outside d_out[0 .. out_capacity) and all index arrays are valid.  *d_n > n_or_capacity (a scan
 * that overflowed): *d_n_snippets = *d_out_symbols = 0 and nothing else is written.  A contract
 * violation -- bad offsets, a record out of range, end_pos decreasing under MERGE -- is handled as
 * replace handles one: a validation pass sees every offset and every record before an address is
 * formed from it, the two counts are 0, d_out and the arrays are untouched, acm_gpu_plan_status
 * reports ACM_GPU_E_INTERNAL and nothing is read or written out of bounds.  d_out must not overlap
 * d_text (ACM_GPU_E_ARG); both may have ANY alignment that is a multiple of the symbol size
 * (replace's 16-byte-word rule: up to 15 bytes in front of and behind a snippet's source are read,
 * never beyond the aligned word that holds a byte of it).  The passes work on tiles of 4,096
 * records (ACM_GPU_CONTEXT_TILE=<records>: a multiple of 64 from 64 to 1 Mi) and the gather on
 * tiles of 16,384 bytes of the output (ACM_GPU_CONTEXT_OUT_TILE=<bytes>: a multiple of 16 from 256
 * to 1 Mi), both read from the environment at every call.  d_tmp must hold
 * acm_gpu_context_tmp_bytes (plan, n_or_capacity, n_texts) bytes: about 20 per record, nothing per
 * symbol or per text (0 for a call that would be refused).
 *
 * acm_gpu_scan_context_device: acm_gpu_scan_ordered_device with emit_from = 0, and the passes above
 * behind it on `stream`; the records stay in d_records[0 .. *d_count).  The capacity rule is
 * select's: `capacity` must hold ALL matches.  *d_count > capacity afterwards: it is the scan's
 * count, *d_n_snippets = *d_out_symbols = 0.  d_tmp must hold acm_gpu_scan_context_tmp_bytes (plan,
 * capacity, n_symbols, n_texts) bytes: the scan's scratch is reused, it has ended when the context
 * passes begin.
 * acm_gpu_scan_context_host: the same from host memory, blocking.  n_found, n_snippets and
 * out_symbols are required; records and every array may be NULL.  ACM_GPU_E_OVERFLOW has
 * acm_gpu_grep_lines_host's two meanings, told apart the same way: *n_found > capacity -- only
 * *n_found is valid --; otherwise *out_symbols > out_capacity -- everything but `out` is valid.
 * Offsets that break the batch contract are ACM_GPU_E_ARG.
 * acm_context: the call on the machine itself, for one text (so TEXTS is ACM_GPU_E_ARG), total over
 * machines exactly as acm_scan_words is (same three paths, same cached plan, acm_scan_path recorded
 * on success and on either overflow): ACM_SCAN_PATH_CPU_LOOP runs the caller loop and then
 * acm_context_records.  A missing device stays an error.
 *
 * Out of scope: context flags inside acm_grep and acm_grep_lines (their signatures do not change);
 * several GPUs, streams and flows; highlight markers written into the output (rec_at gives their
 * places); line numbers (snip_text is the line number under a split). */
#define ACM_CONTEXT_SYMBOLS 0
#define ACM_CONTEXT_TEXTS 1
#define ACM_CONTEXT_EACH 0
#define ACM_CONTEXT_MERGE 2
#define ACM_CONTEXT_NONE 0xFFFFFFFFu
int acm_context_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base,
                         const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                         const ACMRecord *records, uint64_t n, uint32_t before, uint32_t after, uint32_t flags,
                         void *out /* may be NULL */, uint64_t out_capacity, uint64_t *out_symbols,
                         uint64_t *n_snippets, uint64_t *snip_lo, uint64_t *out_offsets,
                         uint32_t *snip_text, uint32_t *rec_snip, int64_t *rec_at);
size_t acm_gpu_context_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_texts);
int acm_gpu_context_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                    const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                    const ACMRecord *d_records, uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                    uint32_t before, uint32_t after, uint32_t flags,
                                    void *d_out /* may be NULL */, uint64_t out_capacity, uint64_t *d_out_symbols,
                                    uint64_t *d_n_snippets, uint64_t *d_snip_lo, uint64_t *d_out_offsets,
                                    uint32_t *d_snip_text, uint32_t *d_rec_snip, int64_t *d_rec_at /* the three may be NULL */,
                                    void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_context_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_context_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                 const uint64_t *d_offsets, uint64_t n_texts,
                                 ACMRecord *d_records, uint64_t capacity, uint64_t *d_count,
                                 uint32_t before, uint32_t after, uint32_t flags,
                                 void *d_out, uint64_t out_capacity, uint64_t *d_out_symbols,
                                 uint64_t *d_n_snippets, uint64_t *d_snip_lo, uint64_t *d_out_offsets,
                                 uint32_t *d_snip_text, uint32_t *d_rec_snip, int64_t *d_rec_at,
                                 void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_context_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                               const uint64_t *offsets, uint64_t n_texts,
                               ACMRecord *records /* may be NULL */, uint64_t capacity, uint64_t *n_found,
                               uint32_t before, uint32_t after, uint32_t flags,
                               void *out, uint64_t out_capacity, uint64_t *out_symbols,
                               uint64_t *n_snippets, uint64_t *snip_lo, uint64_t *out_offsets,
                               uint32_t *snip_text, uint32_t *rec_snip, int64_t *rec_at);   /* blocking */
int acm_context (ACMachine *machine, const void *text, uint64_t n_symbols,
                 ACMRecord *records /* may be NULL */, uint64_t capacity, uint64_t *n_found,
                 uint32_t before, uint32_t after, uint32_t flags,
                 void *out, uint64_t out_capacity, uint64_t *out_symbols,
                 uint64_t *n_snippets, uint64_t *snip_lo, uint64_t *out_offsets,
                 uint32_t *snip_text, uint32_t *rec_snip, int64_t *rec_at);

/* ------------------------------------------------------------------ anchored matches and dictionary lookup
 * Every consumer above rests on the unanchored scan: every occurrence of every keyword anywhere in a
 * text.  The first question asked of table cells, packets and log lines is an anchored one: is this
 * cell a keyword (set membership, dictionary encoding of a column, `grep -x -F -f`), does this line
 * begin with a keyword (a protocol verb, a log tag, a URL scheme), which is the longest keyword it
 * begins with.  It needs no scan: text t is walked from the root along the goto function only -- no
 * failure link -- for at most min (|text t|, lmax) symbols, stopping at the first missing edge.  The
 * cost does not depend on how long the texts are, and the result is bounded by the texts, not by
 * the matches of the buffer.
 *
 * DEFINITION.  Inputs: the batch contract -- text t is the symbols [offsets[t], offsets[t + 1]) of
 * one packed buffer, offsets[0] = 0, offsets[n_texts] = n_symbols, never decreasing, empty texts
 * allowed.  Let B be acm_scan_batch's record set of that batch (the caller loop from acm_initiate on
 * every text alone, end_pos = offsets[t] + i); a record's start is end_pos + 1 - length.
 * ANCHORED (B, offsets, mode).  For every text t, in order, let P_t be the records of text t whose
 * start equals offsets[t] -- the keywords that are prefixes of text t -- by ascending length (the
 * canonical order: they share a start).
 *   ACM_ANCHORED_PREFIXES (1) keeps all of P_t;
 *   ACM_ANCHORED_LONGEST (2) keeps the last record of P_t, if P_t has any;
 *   ACM_ANCHORED_WHOLE (3) keeps the record of P_t whose length is offsets[t + 1] - offsets[t], if
 *     there is one: `grep -x`.
 * Any other mode is ACM_GPU_E_ARG.  An empty text has no record.  The output is the concatenation
 * over t, in canonical order by construction; text_id[r] and first[0 .. n_texts] come beside the
 * records and mean exactly what acm_scan_batch's mean.
 * LOOKUP.  The same walk with one fixed-size answer per text and no records:
 *   whole_id[t]    the keyword_id of WHOLE's record of text t, else ACM_LOOKUP_NONE (0xFFFFFFFF);
 *   prefix_id[t]   the keyword_id of LONGEST's record of text t, else ACM_LOOKUP_NONE;
 *   prefix_len[t]  the length of LONGEST's record of text t, else 0.
 * Each of the three arrays may be NULL; all three NULL is ACM_GPU_E_ARG.  The outputs are SET, not
 * added to.
 * Symbols compare as the plan's scan compares them: a plan of comparator classes matches over
 * classes, an interned 8-byte plan over its ids.  Keyword ids are first-insertion ranks; keywords of
 * a pending delta count like any others.
 *
 * acm_anchored_records: the plain sequential ANCHORED of a batch's records (in canonical order) on
 * the host, no device, in place in the front of the array; text_id and first (each may be NULL) are
 * rewritten for the kept records.  Offsets that break the contract, a record outside
 * [0, offsets[n_texts]), of length 0 or across a cut: ACM_GPU_E_ARG, nothing modified.
 *
 * acm_gpu_scan_anchored_device (dev_anchored.h): the check of d_offsets in a launch of its own, a
 * count pass (one lane per text), a 64-bit prefix sum into first[], a fill pass that walks again.
 * The call only queues launches on `stream`, with no host round trip -- but for the classification
 * round of 4-byte comparator-class plans, which the scans have too: the text goes through the plan's
 * own preparation where that changes what a symbol is (class ids, interned ids) and the walk
 * compares what the scan kernels compare; the aligned copy some plans make of a text for their scan
 * kernels is not made, since the walk reads at most lmax symbols of a text.  A start-parallel plan
 * is walked in the tables acm_gpu_plan_update edits; a plan with a pending delta walks both tries in
 * lockstep.  d_text: any multiple of the caller's symbol size.
 * CAPACITY holds the ANCHORED records only, never the concatenation's matches:
 * min (sum over t of min (len_t, lmax), n_texts x the deepest nesting of keyword prefixes) bounds
 * PREFIXES; LONGEST and WHOLE keep at most one record per text, so capacity = n_texts cannot overflow.
 * *d_count <= capacity: the count is exact, and d_records, d_text_id and d_first are complete.
 * *d_count > capacity: it is the capacity needed, and d_first is complete and valid (as
 * acm_gpu_rules_device's fired_ptr is); d_records and d_text_id are unspecified and nothing is
 * written outside d_records[0 .. capacity).  d_offsets that break the contract: *d_count = 0, no
 * other output, acm_gpu_plan_status reports ACM_GPU_E_INTERNAL; no address is formed from an offset
 * before the check has seen it.  n_texts = 0 requires n_symbols = 0 and gives no record; n_texts >=
 * 2^31 - 1 is ACM_GPU_E_ARG (the prefix sum counts its n_texts + 1 items in 31 bits;
 * acm_gpu_lookup_device, which has none, takes up to 2^32 - 1 texts).  d_tmp must hold acm_gpu_scan_anchored_tmp_bytes (plan,
 * n_texts) bytes (0 for a call that would be refused): about 16 bytes per text.  Any plan kind, not
 * while a stream (acm_gpu_stream_*) is open on the plan, one call at a time per plan.
 * ACM_GPU_ANCHORED_GRID=<blocks> in the environment (1 to 2^20, read at every call) caps the grids
 * of the two passes (tests: a few blocks striding over thousands of texts).
 * acm_gpu_lookup_device: the check and the count pass alone, writing the arrays the caller gave.
 * Under d_offsets that break the contract no output array is written and the status is
 * ACM_GPU_E_INTERNAL.  d_tmp must hold acm_gpu_lookup_tmp_bytes (plan, n_texts) bytes.
 * acm_gpu_scan_anchored_host, acm_gpu_lookup_host: the same from host memory, blocking; offsets[]
 * is checked on the host (ACM_GPU_E_ARG); on ACM_GPU_E_OVERFLOW *n_found holds the capacity needed and
 * first[] (if given) is complete, on every path of acm_scan_anchored too; records and text_id are
 * not written then.
 * acm_scan_anchored, acm_lookup: the calls on the machine itself, total over machines exactly as
 * acm_scan_batch is (same three paths, same cached plan, same acm_gpu_plan_update; acm_scan_path
 * recorded on success and on overflow).  ACM_SCAN_PATH_CPU_LOOP runs the caller loop per text on the
 * host and acm_anchored_records, and derives the lookup arrays from LONGEST and WHOLE.  A missing
 * device stays an error, never a fallback.
 *
 * Out of scope: matches anchored at the END of a text (suffix matches: acm_scan_batch and a host
 * filter); flows, streams and several GPUs; pos_base; anchoring inside acm_grep, acm_tally_batch or
 * acm_rules (their signatures do not change); case folding other than through comparator classes. */
#define ACM_ANCHORED_PREFIXES 1
#define ACM_ANCHORED_LONGEST 2
#define ACM_ANCHORED_WHOLE 3
#define ACM_LOOKUP_NONE 0xFFFFFFFFu
int acm_anchored_records (const uint64_t *offsets, uint64_t n_texts, uint32_t mode,
                          ACMRecord *records, uint64_t n, uint32_t *text_id /* may be NULL */,
                          uint64_t *first /* n_texts + 1, may be NULL */, uint64_t *n_kept);   /* in place, front of the array */
size_t acm_gpu_scan_anchored_tmp_bytes (const ACMPlan *plan, uint64_t n_texts);
int acm_gpu_scan_anchored_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols,
                                  const uint64_t *d_offsets, uint64_t n_texts, uint32_t mode,
                                  ACMRecord *d_records, uint32_t *d_text_id /* may be NULL */,
                                  uint64_t *d_first /* n_texts + 1, may be NULL */,
                                  uint64_t capacity, uint64_t *d_count,
                                  void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_lookup_tmp_bytes (const ACMPlan *plan, uint64_t n_texts);
int acm_gpu_lookup_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols,
                           const uint64_t *d_offsets, uint64_t n_texts,
                           uint32_t *d_whole_id /* may be NULL */, uint32_t *d_prefix_id /* may be NULL */,
                           uint32_t *d_prefix_len /* may be NULL */,
                           void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_anchored_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t mode,
                                ACMRecord *records, uint32_t *text_id, uint64_t *first,
                                uint64_t capacity, uint64_t *n_found);       /* blocking */
int acm_gpu_lookup_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts,
                         uint32_t *whole_id, uint32_t *prefix_id, uint32_t *prefix_len);   /* blocking */
int acm_scan_anchored (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t mode,
                       ACMRecord *records, uint32_t *text_id, uint64_t *first,
                       uint64_t capacity, uint64_t *n_found);
int acm_lookup (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts,
                uint32_t *whole_id, uint32_t *prefix_id, uint32_t *prefix_len);

/* ------------------------------------------------------------------ streaming scan
 * Text that arrives piece by piece from the host (the reference's callers read files symbol by
 * symbol, generic_test.c:191).  The result is the caller loop's output over the concatenation of
 * all pieces fed so far (end_pos = position in the whole stream): the last lmax - 1 symbols are
 * carried over in front of every piece.  Host-to-device copies of a piece overlap with the scan of
 * the previous one (two device slots, two streams).  One open stream per plan at a time; do not
 * mix with acm_gpu_scan_* calls on the same plan while it is open. */
typedef struct ACMStream ACMStream;
int acm_gpu_stream_open (ACMPlan *plan, uint64_t max_piece_symbols, uint64_t record_capacity, ACMStream **out);
/* Enqueues copy + scan of the next n_symbols (split into pieces of at most max_piece_symbols) and
 * returns; `text` (host memory, pinned for a truly asynchronous copy) must stay untouched until
 * the second next feed or acm_gpu_stream_finish. */
int acm_gpu_stream_feed (ACMStream *stream, const void *text, uint64_t n_symbols);
/* Waits, sorts into canonical order, copies the records of the whole stream so far to the host.
 * ACM_GPU_E_OVERFLOW (with *n_found = number needed) if they exceed the stream's or this call's
 * capacity.  The stream stays open. */
int acm_gpu_stream_finish (ACMStream *stream, ACMRecord *records, uint64_t capacity, uint64_t *n_found);
void acm_gpu_stream_close (ACMStream *stream);

/* ------------------------------------------------------------------ keyword patterns with don't-care gaps
 * Every consumer above acts on whole keywords; acm_rules combines them per text but knows no
 * position.  A pattern with don't-care symbols -- a hex signature `E2 34 ?? C8 A1`, a motif with N, a
 * fixed-column record template -- is the textbook second use of the automaton: the pattern is cut
 * into its fragments, the fragments are the dictionary, and an occurrence of the pattern is a set of
 * fragment occurrences at fixed distances from each other.  PATTERNS is that join.  It is a pure
 * function of a record set in canonical order, as WORDS and SELECT are, so it runs behind every plan
 * kind, symbol size, class plan and pending delta alike and has the record passes' calling shape.
 *
 * DEFINITION.  Terms and patterns: an ACMPatternTerm is (keyword_id, offset, length), three uint32_t.
 * Pattern p is the terms [pat_ptr[p], pat_ptr[p + 1]) of terms[]; pat_ptr has n_patterns + 1 uint64_t
 * entries.  A term says: keyword keyword_id, which is `length` symbols long, begins `offset` symbols
 * behind the pattern's first symbol.  The pattern's length is L_p = max over its terms of (offset +
 * length).  Symbols covered by no term are don't-cares.  Terms may come in any order and may
 * overlap; leading don't-cares are allowed (the smallest offset may be above 0).
 * ACM_GPU_E_ARG: a pattern without terms, length == 0, offset + length >= 2^31, keyword_id >=
 * n_keywords, a pat_ptr that decreases or does not begin with 0, n_patterns >= 2^31, 2^31 terms or
 * more.
 * PATTERNS (R, offsets, P).  R is a record set in canonical order with positions pos_base + index.
 * Text t is [offsets[t], offsets[t + 1]) under the batch contract (first 0, last n_symbols, never
 * decreasing, empty texts allowed); offsets == NULL means that the buffer [0, n_symbols) is one
 * text.  Pattern p MATCHES at buffer index S iff
 *   there is a text t with offsets[t] <= S and S + L_p <= offsets[t + 1], and
 *   for every term (k, o, l) of p the record (pos_base + S + o + l - 1, l, k) is in R.
 * Each match gives one ACMRecord (end_pos = pos_base + S + L_p - 1, length = L_p, keyword_id = p).
 * The output is in the total order end_pos ascending, then length descending, then pattern id
 * ascending: deterministic, whichever term an implementation anchors on.  A term whose `length` is
 * not its keyword's length never holds; the record passes cannot know the lengths, so this is no
 * error in them.  Records that span a cut never take part, because every term lies inside
 * [S, S + L_p): PATTERNS of the ordered scan of the packed buffer equals PATTERNS of
 * acm_scan_batch's records.  When the terms of every pattern are the maximal don't-care-free runs of
 * a template, this is exactly every occurrence, overlapping ones included, of the template with each
 * don't-care matching any one symbol, inside one text; symbols compare as the plan's scan compares
 * them.
 *
 * acm_patterns_check: the argument checks above, no device; every other entry point runs it.
 * acm_patterns_records: the plain sequential PATTERNS on the host, no device.  ACM_GPU_E_OVERFLOW
 * with *n_found = the entries needed when out_capacity is too small; `out` is untouched then.
 * out == NULL with capacity 0 only counts.  ACM_GPU_E_ARG, with nothing written, for offsets that
 * break the batch contract and for a record outside [pos_base, pos_base + n_symbols) (its end or
 * its start) or of length 0.
 *
 * acm_gpu_patterns_create compiles a set once on the host and uploads it to the plan's device
 * (ACMPatterns, opaque like ACMRules).  Each pattern's ANCHOR is the term with the greatest offset +
 * length, the lowest index among equals: the anchor's match ends where the pattern's does.  The
 * compiled set is an index inverted by anchor keyword, each keyword's postings sorted by (L
 * descending, pattern id ascending), and per pattern its terms as (distance of the term's end in
 * front of the pattern's end, length, keyword_id).  n_keywords is acm_gpu_tally_keywords (plan) at
 * creation; the set stays valid after acm_gpu_plan_update, as a rule set does.
 * acm_gpu_patterns_info: patterns, terms, the keywords that anchor a pattern, the longest L_p and the
 * most postings of one keyword.  n x max_anchor_postings bounds the output of n records, so a caller
 * can pick an out_capacity that cannot overflow.
 *
 * acm_gpu_patterns_records_device (dev_patterns.h): PATTERNS of d_records on the device,
 * acm_gpu_words_records_device's shape: d_n NULL -- n_or_capacity is the number of records; d_n
 * given -- *d_n is, and n_or_capacity the room of d_records.  n_or_capacity, out_capacity and
 * n_texts are below 2^31; d_out must not overlap d_records (ACM_GPU_E_ARG).  The call only queues
 * launches on `stream`, with no host round trip; the plan is used for its device, its grid cap and
 * its error word only.  The check of d_offsets in a launch of its own (no address is formed from an
 * offset before the check has seen it); a count pass, one lane per input record over tiles of 4,096
 * records (ACM_GPU_PATTERNS_TILE=<records> in the environment sets another: a multiple of 64 from 64
 * to 1 Mi, read at every call) -- the lane reads its keyword's postings and, per posting, tests the
 * anchor term's length, finds the text of S by a bisection of offsets[], tests both bounds and looks
 * every other term up in d_records by its key (end_pos, length), which is unique in canonical order;
 * a 64-bit exclusive sum over the counts; a fill pass that verifies again and writes each match at
 * its slot, one 16-byte store; an order pass that puts every group of equal end_pos into (L
 * descending, pattern id ascending) -- matches of one end can come from several anchor records.  No
 * atomics decide a slot, every output slot is written by one lane, and launch geometry never depends
 * on what the records hold.  d_tmp must hold acm_gpu_patterns_tmp_bytes (plan, patterns,
 * n_or_capacity, n_texts) bytes (0 for a call that would be refused).
 *   *d_count <= out_capacity: the count is exact and d_out is complete and in order.
 *   *d_count > out_capacity: it is the capacity needed, d_out is unspecified, and nothing is written
 *     outside d_out[0 .. out_capacity).
 *   *d_n > n_or_capacity (a scan that overflowed): *d_count = 0 and nothing is written.
 *   d_offsets that break the contract: *d_count = 0, no other output, acm_gpu_plan_status reports
 *     ACM_GPU_E_INTERNAL.
 * A record that breaks the contract (a position outside [pos_base, pos_base + n_symbols), a start
 * below pos_base, a length of 0) is skipped and acm_gpu_plan_status reports ACM_GPU_E_INTERNAL
 * (select's rule).  Input that is not in canonical order gives an unspecified result; nothing is
 * read or written out of bounds.
 *
 * acm_gpu_scan_patterns_device: acm_gpu_scan_ordered_device (emit_from 0) into `capacity` records
 * inside d_tmp, then the passes above; d_tmp must hold acm_gpu_scan_patterns_tmp_bytes (plan,
 * patterns, capacity, n_symbols, n_texts) bytes.  *d_found receives the scan's count: when it
 * exceeds `capacity`, *d_count = 0 and *d_found is a capacity that suffices.
 * acm_gpu_scan_patterns_host: the same from host memory, blocking; it creates and destroys the set
 * itself and sizes the record room from acm_gpu_count_device.  ACM_GPU_E_OVERFLOW means only
 * "out_capacity is too small, *n_found suffices".  Offsets that break the batch contract are
 * ACM_GPU_E_ARG.
 * acm_scan_patterns: the call on the machine itself, total over machines exactly as acm_rules is
 * (same three paths, same cached plan, same acm_gpu_plan_update; acm_scan_path recorded on success
 * and on overflow).  ACM_SCAN_PATH_CPU_LOOP runs the caller loop per text on the host, then
 * acm_patterns_records.  This call knows the machine: a term whose `length` is not its keyword's
 * length is ACM_GPU_E_ARG here.  A missing device stays an error, never a fallback.
 *
 * Out of scope: trailing don't-cares (not expressible: they would test nothing but that the text
 * goes on); bounded variable gaps ({n-m}: acm_scan_chains below joins those); symbol classes inside a pattern (TEMPLATES, the section
 * behind acm_scan_chains, has them) and alternatives (AA|BB); flows,
 * streams and several GPUs; feeding pattern records to SELECT or REPLACE (their contract bounds
 * lengths by the plan's lmax, and L_p is not bound by it). */
typedef struct {
  uint32_t keyword_id, offset, length;
} ACMPatternTerm;
typedef struct ACMPatterns ACMPatterns;
typedef struct {
  uint64_t patterns, terms, anchor_keywords, longest, max_anchor_postings;
} ACMPatternsInfo;
int acm_patterns_check (const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, uint64_t n_keywords);
int acm_patterns_records (const ACMRecord *records, uint64_t n, uint64_t n_symbols, uint64_t pos_base,
                          const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                          const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, uint64_t n_keywords,
                          ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);
int acm_gpu_patterns_create (ACMPlan *plan, const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns,
                             ACMPatterns **out);
void acm_gpu_patterns_destroy (ACMPatterns *patterns);
int acm_gpu_patterns_info (const ACMPatterns *patterns, ACMPatternsInfo *info);
size_t acm_gpu_patterns_tmp_bytes (const ACMPlan *plan, const ACMPatterns *patterns, uint64_t n_or_capacity, uint64_t n_texts);
int acm_gpu_patterns_records_device (ACMPlan *plan, const ACMPatterns *patterns, const ACMRecord *d_records,
                                     uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                     uint64_t n_symbols, uint64_t pos_base,
                                     const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                     ACMRecord *d_out, uint64_t out_capacity, uint64_t *d_count,
                                     void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_patterns_tmp_bytes (const ACMPlan *plan, const ACMPatterns *patterns, uint64_t capacity,
                                        uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_patterns_device (ACMPlan *plan, const ACMPatterns *patterns, const void *d_text, uint64_t n_symbols,
                                  uint64_t pos_base, const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                  uint64_t capacity, ACMRecord *d_out, uint64_t out_capacity,
                                  uint64_t *d_count, uint64_t *d_found, void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_patterns_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                                const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                                const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns,
                                ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);   /* blocking */
int acm_scan_patterns (ACMachine *machine, const void *text, uint64_t n_symbols,
                       const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                       const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns,
                       ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ keywords with up to k mismatches
 * Every consumer above acts on exact occurrences.  APPROX gives approximate ones: every place where a
 * target occurs with at most k substituted symbols (Hamming distance) -- typo-tolerant term lists, primers
 * and motifs with mismatches, signatures with a few variable bytes at unknown positions.  The textbook
 * construction: a target of L symbols with budget k is cut into k + 1 disjoint pieces; wherever the target
 * occurs with at most k mismatches, at least one piece occurs exactly.  So the pieces are the dictionary,
 * every exact piece record is a SEED, and the seed's target is verified against the text around it.  The
 * scan kernels stay untouched; APPROX is a function of a record set in canonical order, of the text and of
 * offsets[], and has the record passes' calling shape.
 *
 * DEFINITION.  Targets: there are n_targets targets.  Target w has a spelling, the symbols
 * [spell_off[w], spell_off[w + 1]) of spell_data in the caller's symbol size (spell_off has n_targets + 1
 * uint64_t entries); its length is L_w.  It has a budget k[w] (uint32_t) and the terms
 * [tgt_ptr[w], tgt_ptr[w + 1]) of terms[] (ACMPatternTerm reused: keyword_id, offset, length).  A term says:
 * keyword keyword_id, `length` symbols long, is the piece of the spelling that begins at `offset`.
 * ACM_GPU_E_ARG: a target without terms, L_w == 0 or L_w >= 2^31, k[w] > 255, a term with length == 0 or
 * offset + length > L_w, keyword_id >= n_keywords, a spell_off or tgt_ptr that decreases or does not begin
 * with 0, n_targets >= 2^31, 2^31 terms or more.
 * APPROX (R, text, offsets, T).  R is a record set in canonical order with positions pos_base + index;
 * text[0 .. n_symbols) is the buffer in the caller's symbols; offsets follows the batch contract (NULL:
 * one text).  Target w MATCHES at buffer index S iff
 *   1. some text t has offsets[t] <= S and S + L_w <= offsets[t + 1], and
 *   2. (seed) some term (kid, o, l) of w has the record (pos_base + S + o + l - 1, l, kid) in R, and
 *   3. d = the number of i < L_w with text[S + i] != spell_w[i] is <= k[w]; symbols compare bitwise over
 *      sym_bytes bytes.
 * Each (w, S) that matches gives exactly one ACMRecord (end_pos = pos_base + S + L_w - 1, length = L_w,
 * keyword_id = w) and dist[r] = d, however many terms seed it.  The total order is end_pos ascending, then
 * length descending, then target id ascending.
 * COMPLETENESS.  When the terms of w are k[w] + 1 pairwise disjoint pieces, each keyword is spelled exactly
 * as its piece and R is the full record set of the buffer, condition 2 follows from 1 and 3: APPROX is
 * then every occurrence of every target within its budget, inside one text.  acm_approx_split (L, k, j)
 * gives the canonical cut: piece j is [floor (j * L / (k + 1)), floor ((j + 1) * L / (k + 1))); it needs
 * L >= k + 1 and j <= k (ACM_GPU_E_ARG otherwise).  With fewer terms, or terms that are not such pieces,
 * the seed condition removes matches; that is defined, not an error.
 *
 * acm_approx_check: the argument checks above, no device; every other entry point runs it.
 * acm_approx_records: the plain sequential APPROX on the host, no device.  ACM_GPU_E_OVERFLOW with
 * *n_found = the entries needed, and nothing written, when out_capacity is too small; out == NULL with
 * capacity 0 only counts; `dist` may be NULL.  ACM_GPU_E_ARG, with nothing written, for offsets that break
 * the batch contract and for a record outside [pos_base, pos_base + n_symbols) (its end or its start) or
 * of length 0.
 *
 * acm_gpu_approx_create compiles a set once on the host and uploads it to the plan's device (ACMApprox,
 * opaque like ACMPatterns): an index inverted by term keyword with postings (target id, term index j,
 * offset, term length) sorted by (target id, j), per target its terms, the spellings and the budgets.
 * n_keywords is acm_gpu_tally_keywords (plan) at creation; the set stays valid after acm_gpu_plan_update.
 * A plan over comparator classes is refused with ACM_GPU_E_INELIGIBLE, because verification is bitwise on
 * the caller's text; plans that intern 8-byte symbols are taken, since interning is exact.
 * acm_gpu_approx_info: targets, terms, the keywords that seed a target, the longest L_w, the largest k and
 * the most postings of one keyword; n x max_postings bounds the output of n records.
 *
 * acm_gpu_approx_records_device (dev_approx.h): APPROX of d_records on the device, the shape of
 * acm_gpu_patterns_records_device (d_n, n_or_capacity, overlap rule, 2^31 limits) plus d_text -- the
 * caller's symbols at any address that is a multiple of the symbol size -- and d_dist (uint32_t per
 * output entry, may be NULL).  It only queues launches, with no host round trip.  The check of d_offsets
 * in a launch of its own; a count pass with one group of 16 consecutive lanes per input record over tiles
 * of 1,024 records (ACM_GPU_APPROX_TILE=<records>: a multiple of 64 from 64 to 1 Mi, read at every call):
 * the group reads the postings of the record's keyword and per posting tests the term's length, S >= 0,
 * the text of S by a bisection of offsets[] and that S + L_w ends inside it, verifies cooperatively --
 * lane j compares symbols j, j + 16, ... with naturally aligned loads of one symbol, the mismatches grow
 * by the popcount of the group's 16 bits of the wave's ballot, and the group stops once they exceed k[w]
 * -- and drops a candidate within its budget when a term of lower index of the same target also has its
 * record in R (that term's group emits the match); a 64-bit exclusive sum; a fill pass in which the groups with a
 * nonzero count verify again and store each match with one 16-byte store plus its distance; an order
 * pass, run only when the total fits out_capacity -- two stable radix sorts (hipCUB) of an index
 * permutation, by (length descending, target id) and then by end_pos - pos_base, and one gather of
 * records and distances.  No atomics decide a slot and launch geometry never depends on what the records
 * hold.  d_tmp must hold acm_gpu_approx_tmp_bytes (plan, approx, n_or_capacity, out_capacity, n_texts)
 * bytes (0 for a call that would be refused).
 *   *d_count <= out_capacity: the count is exact, d_out and d_dist are complete and in order.
 *   *d_count > out_capacity: it is the capacity needed, and nothing is written to d_out or d_dist.
 *   *d_n > n_or_capacity (a scan that overflowed): *d_count = 0 and nothing is written.
 *   d_offsets that break the contract: *d_count = 0, no other output, acm_gpu_plan_status reports
 *     ACM_GPU_E_INTERNAL.
 * A record that breaks the contract (a position outside [pos_base, pos_base + n_symbols), a start below
 * pos_base, a length of 0) is skipped and acm_gpu_plan_status reports ACM_GPU_E_INTERNAL (select's
 * rule).  Input that is not in canonical order gives an unspecified result; nothing is read or written
 * out of bounds.
 *
 * acm_gpu_scan_approx_device: acm_gpu_scan_ordered_device (emit_from 0) into `capacity` records inside
 * d_tmp, then the passes above; d_tmp must hold acm_gpu_scan_approx_tmp_bytes (plan, approx, capacity,
 * out_capacity, n_symbols, n_texts) bytes.  *d_found receives the scan's count: when it exceeds
 * `capacity`, *d_count = 0 and *d_found is a capacity that suffices.
 * acm_gpu_scan_approx_host: the same from host memory, blocking; it creates and destroys the set itself
 * and sizes the record room from acm_gpu_count_device.  ACM_GPU_E_OVERFLOW means only "out_capacity is
 * too small, *n_found suffices".  Offsets that break the batch contract are ACM_GPU_E_ARG.
 * acm_scan_approx: the call on the machine itself.  This call knows the machine: a term whose length or
 * spelling is not that of its keyword's piece is ACM_GPU_E_ARG.  Machines with ACM_CMP_DEFAULT run the
 * GPU path; machines with another comparator run the caller loop on the host and the sequential join
 * with symbols compared by the machine's comparator, report ACM_SCAN_PATH_CPU_LOOP and need
 * acm_set_symbol_bytes (ACM_GPU_E_INELIGIBLE without it).  A missing device stays an error, never a
 * fallback.
 *
 * Out of scope: insertions and deletions (edit distance: EDIT, the next section); positions that take one
 * of several symbols (TEMPLATES, the section behind acm_scan_chains); class plans on the
 * device; flows, streams and several GPUs; feeding the output to SELECT or REPLACE (their contract bounds
 * lengths by the plan's lmax, and L_w is not bound by it). */
typedef struct ACMApprox ACMApprox;
typedef struct {
  uint64_t targets, terms, seed_keywords, longest, max_k, max_postings;
} ACMApproxInfo;
int acm_approx_check (const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr,
                      uint64_t n_targets, uint64_t n_keywords);
int acm_approx_split (uint64_t L, uint32_t k, uint32_t j, uint64_t *begin, uint64_t *end);
int acm_approx_records (const ACMRecord *records, uint64_t n, const void *text, uint32_t sym_bytes, uint64_t n_symbols,
                        uint64_t pos_base, const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                        const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                        const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets, uint64_t n_keywords,
                        ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity, uint64_t *n_found);
int acm_gpu_approx_create (ACMPlan *plan, const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                           const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets, ACMApprox **out);
void acm_gpu_approx_destroy (ACMApprox *approx);
int acm_gpu_approx_info (const ACMApprox *approx, ACMApproxInfo *info);
size_t acm_gpu_approx_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t n_or_capacity,
                                 uint64_t out_capacity, uint64_t n_texts);
int acm_gpu_approx_records_device (ACMPlan *plan, const ACMApprox *approx, const ACMRecord *d_records,
                                   uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                   const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                   const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                   ACMRecord *d_out, uint32_t *d_dist /* may be NULL */, uint64_t out_capacity,
                                   uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_approx_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t capacity,
                                      uint64_t out_capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_approx_device (ACMPlan *plan, const ACMApprox *approx, const void *d_text, uint64_t n_symbols,
                                uint64_t pos_base, const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                uint64_t capacity, ACMRecord *d_out, uint32_t *d_dist /* may be NULL */,
                                uint64_t out_capacity, uint64_t *d_count, uint64_t *d_found,
                                void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_approx_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                              const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                              const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                              const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets,
                              ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity,
                              uint64_t *n_found);   /* blocking */
int acm_scan_approx (ACMachine *machine, const void *text, uint64_t n_symbols,
                     const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                     const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                     const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets,
                     ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ keywords within edit distance k
 * APPROX survives substituted symbols only.  EDIT also survives a dropped and an added symbol: every end
 * at which a target occurs within unit-cost Levenshtein distance k -- the typos of a term list (`Daloway`
 * is at Hamming distance 6 of `Dalloway`, and at edit distance 1), indels in primers and motifs, a byte
 * inserted into a signature.  The compiled set is APPROX's (ACMApprox, acm_gpu_approx_create / _destroy /
 * _info): the metric is a property of the call.  The cut into k + 1 pieces is complete for edit distance
 * too; what differs is the verification, because a seed no longer fixes one start: it fixes up to
 * 2 k + 1 ends and a band of start diagonals.
 *
 * DEFINITION.  Targets, spellings, budgets and terms are exactly APPROX's: spell_data, spell_off, k,
 * terms, tgt_ptr, n_targets.  The edit calls add two conditions (acm_edit_check; ACM_GPU_E_ARG
 * otherwise): k[w] <= 15, and k[w] < L_w, so that no match is empty.
 * EDIT (R, text, offsets, T).  R is a record set in canonical order with positions pos_base + index;
 * text[0 .. n_symbols) is in the caller's symbols; offsets follows the batch contract (NULL: one text);
 * symbols compare bitwise over sym_bytes bytes.  For a target w with spelling P (L symbols) and a text
 * [lo, hi):
 *   ed (P, X) is the unit-cost Levenshtein distance: substitution, insertion and deletion cost 1 each;
 *   for a buffer index e in [lo, hi), D_w (e) = min over s in [lo, e + 1] of ed (P, text[s .. e]);
 *   s*_w (e) is the LARGEST s that attains the minimum: the shortest best match.  With D <= k < L it has
 *   e - s* + 1 >= L - k >= 1.
 * Target w MATCHES with end e iff
 *   1. D_w (e) <= k[w], and
 *   2. (seed) some term (kid, o, l) of w, with r = L_w - o - l the symbols of the target behind the piece,
 *      has a record (pos_base + q, l, kid) in R with lo <= q - l + 1 and q < hi (the piece lies inside
 *      the text of e) and max (0, r - k[w]) <= e - q <= r + k[w].
 * Each (w, e) that matches gives exactly one ACMRecord (end_pos = pos_base + e, length = e - s*_w (e) + 1,
 * keyword_id = w) and dist[...] = D_w (e), however many terms and records seed it.  The total order is
 * end_pos ascending, then length descending, then target id ascending.
 * COMPLETENESS.  When the terms of w are k[w] + 1 pairwise disjoint pieces, each keyword is spelled as its
 * piece and R is the full record set of the buffer, condition 2 follows from condition 1.  Proof: an
 * alignment of P with text[s* .. e] of cost D <= k touches at most k of the k + 1 disjoint pieces, so one
 * piece [o, o + l) is aligned symbol by symbol with equal text symbols text[q - l + 1 .. q], s* <= q - l + 1
 * and q <= e; that is an exact occurrence of the keyword inside the text of e, so its record is in R.  The
 * r symbols of P behind the piece are aligned with text(q .. e], whose e - q symbols differ from r by at
 * most the insertions and deletions of the alignment: |e - q - r| <= k, and e - q >= 0.  EDIT is then
 * every end, inside one text, at which the target occurs within its budget: the textbook (Sellers)
 * semantics.  Neighbouring ends e - 1, e, e + 1 of one occurrence are all reported when all are within
 * the budget; that is the definition.  With fewer terms, or terms that are not such pieces, condition 2
 * removes matches; that is defined, not an error.
 *
 * acm_edit_check: acm_approx_check plus the two conditions.  acm_edit_records: the plain sequential EDIT
 * on the host, no device, acm_approx_records' contract; its work follows the seeds: per seed the banded
 * dynamic programme of its window, then the hits in order with each (w, e) kept once.
 * acm_gpu_edit_records_device (dev_edit.h): acm_gpu_approx_records_device's contract, word for word,
 * with these differences.  A set with max_k > 15 or a target of L_w <= k[w] is refused (ACM_GPU_E_ARG,
 * and the tmp_bytes calls return 0); the set remembers at creation whether it is fit for EDIT.
 * acm_gpu_approx_info's figures bound the output: n records give at most n x max_postings x
 * (2 max_k + 1) matches.  One group of G consecutive lanes takes one input record, G = 16, 32 or 64 for
 * max_k <= 3, 7 or 15, over tiles of 64 records (ACM_GPU_EDIT_TILE=<records>: a multiple of 64 from 64
 * to 1 Mi, read at every call).  Per posting the group runs the cheap tests, then the banded dynamic
 * programme with one lane per diagonal as an anti-diagonal wavefront with Ukkonen's cut-off, and a match
 * (w, e) is emitted by its OWNER alone: the least (term index, record end) among the seeds that satisfy
 * condition 2 for e, decided by lookups in R -- so *d_count is exact in every case, also above
 * out_capacity, and no atomic decides a slot.  The passes are APPROX's: the check of d_offsets in a launch
 * of its own, count, a 64-bit exclusive sum, fill (verifying again), and the order passes only when the
 * total fits.  *d_n > n_or_capacity, bad offsets, records that break the contract and input not in
 * canonical order: APPROX's rules.
 * acm_gpu_scan_edit_device, acm_gpu_scan_edit_host, acm_scan_edit: as their APPROX counterparts.  Class
 * plans are refused with ACM_GPU_E_INELIGIBLE; plans that intern 8-byte symbols are taken.  acm_scan_edit
 * is total over machines as acm_scan_approx is: machines with another comparator run the caller loop and
 * the sequential EDIT under that comparator, report ACM_SCAN_PATH_CPU_LOOP and need acm_set_symbol_bytes;
 * its machine-knowing check is acm_scan_approx's plus the two conditions.
 *
 * Out of scope: thinning neighbouring ends of one occurrence to one match; transpositions at cost 1;
 * weighted costs; k > 15; class plans on the device; flows, streams and several GPUs. */
int acm_edit_check (const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr,
                    uint64_t n_targets, uint64_t n_keywords);
int acm_edit_records (const ACMRecord *records, uint64_t n, const void *text, uint32_t sym_bytes, uint64_t n_symbols,
                      uint64_t pos_base, const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                      const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                      const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets, uint64_t n_keywords,
                      ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity, uint64_t *n_found);
size_t acm_gpu_edit_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t n_or_capacity,
                               uint64_t out_capacity, uint64_t n_texts);
int acm_gpu_edit_records_device (ACMPlan *plan, const ACMApprox *approx, const ACMRecord *d_records,
                                 uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                 const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                 const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                 ACMRecord *d_out, uint32_t *d_dist /* may be NULL */, uint64_t out_capacity,
                                 uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_edit_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t capacity,
                                    uint64_t out_capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_edit_device (ACMPlan *plan, const ACMApprox *approx, const void *d_text, uint64_t n_symbols,
                              uint64_t pos_base, const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                              uint64_t capacity, ACMRecord *d_out, uint32_t *d_dist /* may be NULL */,
                              uint64_t out_capacity, uint64_t *d_count, uint64_t *d_found,
                              void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_edit_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                            const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                            const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                            const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets,
                            ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity,
                            uint64_t *n_found);   /* blocking */
int acm_scan_edit (ACMachine *machine, const void *text, uint64_t n_symbols,
                   const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                   const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                   const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets,
                   ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ keyword chains with bounded gaps
 * PATTERNS joins keyword records at fixed distances.  Most multi-part signatures leave the distance
 * open inside bounds: `content:"A"; content:"B"; distance:2; within:40;`, a motif `C-x(2,4)-C-x(3)-H`,
 * "term A, then term B within n symbols in the same line".  CHAINS is that join.  It is a pure function
 * of a record set in canonical order, as PATTERNS is, so it runs behind every plan kind, symbol size,
 * class plan and pending delta alike and has the record passes' calling shape.
 *
 * DEFINITION.  Terms and chains: an ACMChainTerm is (keyword_id, gap_min, gap_max), three uint32_t.
 * Chain c is the terms [chain_ptr[c], chain_ptr[c + 1]) of terms[], in order; chain_ptr has n_chains +
 * 1 uint64_t entries.  Term j >= 1 says: an occurrence of its keyword begins at least gap_min and at
 * most gap_max symbols behind the last symbol of the occurrence chosen for term j - 1; gap 0 means
 * adjacent.  Terms of one chain never overlap.
 * ACM_GPU_E_ARG: a chain without terms, more than ACM_CHAIN_TERMS_MAX (16) terms, gap_min > gap_max,
 * gap_max > ACM_CHAIN_GAP_MAX (2^20), a first term whose gaps are not 0, 0, keyword_id >= n_keywords,
 * a chain_ptr that decreases or does not begin with 0, n_chains >= 2^31, 2^31 terms or more.
 * CHAINS (R, offsets, C).  R is a record set in canonical order with positions pos_base + index.
 * Texts are as in PATTERNS: offsets == NULL means one text, empty texts are allowed.  An EMBEDDING of
 * chain c with m terms is a list of records r_0 .. r_{m-1} of R such that
 *   r_j has the keyword of term j,
 *   with s_j = end_j + 1 - length_j: gap_min_j <= s_j - end_{j-1} - 1 <= gap_max_j for j >= 1, and
 *   one text holds both s_0 and end_{m-1}.
 * For every pair (c, e) such that an embedding of c with end_{m-1} = e exists the output holds exactly
 * one ACMRecord (end_pos = pos_base + e, length = e + 1 - S, keyword_id = c), S the greatest s_0 among
 * those embeddings: the shortest match that ends at e, the way acm_scan_edit reports.  The output is
 * in the total order end_pos ascending, length descending, chain id ascending.  A chain of one term
 * gives its keyword's records; a chain whose gaps all have gap_min == gap_max gives exactly PATTERNS of
 * the equivalent fixed-offset pattern.  The definition permits a dynamic programme over the term
 * levels -- B_0 (r) = s (r), B_j (r) = the greatest B_{j-1} (r') over the records r' of term j - 1's
 * keyword that end inside r's window [s - 1 - gap_max_j, s - 1 - gap_min_j] -- with the text test made
 * once at the end, on S: a smaller s_0 lies in no later text.
 *
 * acm_chains_check: the argument checks above, no device; every other entry point runs it.
 * acm_chains_records: the plain sequential CHAINS on the host, no device, acm_patterns_records'
 * calling shape: ACM_GPU_E_OVERFLOW with *n_found = the entries needed when out_capacity is too small
 * (`out` is untouched then), out == NULL with capacity 0 only counts, ACM_GPU_E_ARG with nothing
 * written for offsets that break the batch contract and for a record outside [pos_base, pos_base +
 * n_symbols) (its end or its start) or of length 0.
 *
 * acm_gpu_chains_create compiles a set once on the host and uploads it to the plan's device
 * (ACMChains, opaque like ACMPatterns): an index inverted by keyword.  A keyword's postings are
 * (chain, level j, gap_min, gap_max, the keyword of term j - 1, the index of the posting (chain, j - 1)
 * among that keyword's postings, a last-term flag), by level, then chain.  n_keywords is
 * acm_gpu_tally_keywords (plan) at creation; the set stays valid after acm_gpu_plan_update, and a
 * keyword added later chains nothing.
 * acm_gpu_chains_info: chains, terms, the most terms of a chain, the widest gap_max, the most
 * postings of one keyword and the most last-term postings of one keyword.  n x max_last_postings
 * bounds the output of n records, so a caller can pick an out_capacity that cannot overflow.
 *
 * acm_gpu_chains_records_device (dev_chains.h): CHAINS of d_records on the device,
 * acm_gpu_patterns_records_device's contract: d_n NULL -- n_or_capacity is the number of records; d_n
 * given -- *d_n is, and n_or_capacity the room of d_records.  n_or_capacity, out_capacity and n_texts
 * are below 2^31 (and n_or_capacity x max_postings below 2^40); d_out must not overlap d_records
 * (ACM_GPU_E_ARG).  The call only queues launches on `stream`, with no host round trip; the plan is
 * used for its device, its grid cap and its error word only.  The check of d_offsets in a launch of
 * its own; then one LEVEL PASS per term level of the set (max_terms launches, at most 16): every
 * record has one state slot per posting of its keyword (a fixed stride of max_postings slots), a slot
 * holds the best start or "none", and pass j fills the slots of level-j postings from the level-(j - 1)
 * slots the launch before wrote -- one bisection of d_records for the window's first record, then a
 * walk forward.  A window of up to T records is walked by its own lane; a wider one by the whole wave,
 * one such lane at a time, 64 records per 16-byte-per-lane load, the maximum reduced across the wave.
 * T is 64 (ACM_GPU_CHAINS_COOP=<records> in the environment sets another, read at every call: 0
 * makes every window cooperative, a huge value none; both forms give the same output).  Then a count
 * pass over the last-term slots (with the text test on S), a 64-bit exclusive sum, a fill pass and
 * PATTERNS' order pass over every group of equal end_pos.  Tiles of 4,096 records
 * (ACM_GPU_CHAINS_TILE=<records>: a multiple of 64 from 64 to 1 Mi, read at every call).  No atomics
 * decide a slot, every slot is written by one lane, and launch geometry and launch count depend on the
 * set, never on what the records hold.  d_tmp must hold acm_gpu_chains_tmp_bytes (plan, chains,
 * n_or_capacity, n_texts) bytes (0 for a call that would be refused).
 *   *d_count <= out_capacity: the count is exact and d_out is complete and in order.
 *   *d_count > out_capacity: it is the capacity needed, d_out is unspecified, and nothing is written
 *     outside d_out[0 .. out_capacity).
 *   *d_n > n_or_capacity (a scan that overflowed): *d_count = 0 and nothing is written.
 *   d_offsets that break the contract: *d_count = 0, no other output, acm_gpu_plan_status reports
 *     ACM_GPU_E_INTERNAL.
 * A record that breaks the contract (a position outside [pos_base, pos_base + n_symbols), a start
 * below pos_base, a length of 0) is skipped -- it ends no chain and takes part in none -- and
 * acm_gpu_plan_status reports ACM_GPU_E_INTERNAL (select's rule).  Input that is not in canonical
 * order gives an unspecified result; nothing is read or written out of bounds.
 *
 * acm_gpu_scan_chains_device: acm_gpu_scan_ordered_device (emit_from 0) into `capacity` records
 * inside d_tmp, then the passes above; d_tmp must hold acm_gpu_scan_chains_tmp_bytes (plan, chains,
 * capacity, n_symbols, n_texts) bytes.  *d_found receives the scan's count: when it exceeds
 * `capacity`, *d_count = 0 and *d_found is a capacity that suffices.
 * acm_gpu_scan_chains_host: the same from host memory, blocking; it creates and destroys the set
 * itself and sizes the record room from acm_gpu_count_device.  ACM_GPU_E_OVERFLOW means only
 * "out_capacity is too small, *n_found suffices".  Offsets that break the batch contract are
 * ACM_GPU_E_ARG.
 * acm_scan_chains: the call on the machine itself, total over machines exactly as acm_scan_patterns
 * is (same three paths, same cached plan, same acm_gpu_plan_update; acm_scan_path recorded on success
 * and on overflow).  ACM_SCAN_PATH_CPU_LOOP runs the caller loop per text on the host, then
 * acm_chains_records.  A missing device stays an error, never a fallback.
 *
 * Out of scope: negative gaps and overlapping terms; symbol classes inside a gap (unordered
 * proximity, NEAR, is acm_near.h's); all embeddings rather than one record per end; flows, streams and several GPUs;
 * feeding chain records to SELECT or REPLACE (their contract bounds lengths by the plan's lmax). */
#define ACM_CHAIN_TERMS_MAX 16u
#define ACM_CHAIN_GAP_MAX (1u << 20)
typedef struct {
  uint32_t keyword_id, gap_min, gap_max;
} ACMChainTerm;
typedef struct ACMChains ACMChains;
typedef struct {
  uint64_t chains, terms, max_terms, max_gap, max_postings, max_last_postings;
} ACMChainsInfo;
int acm_chains_check (const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, uint64_t n_keywords);
int acm_chains_records (const ACMRecord *records, uint64_t n, uint64_t n_symbols, uint64_t pos_base,
                        const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                        const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, uint64_t n_keywords,
                        ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);
int acm_gpu_chains_create (ACMPlan *plan, const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains,
                           ACMChains **out);
void acm_gpu_chains_destroy (ACMChains *chains);
int acm_gpu_chains_info (const ACMChains *chains, ACMChainsInfo *info);
size_t acm_gpu_chains_tmp_bytes (const ACMPlan *plan, const ACMChains *chains, uint64_t n_or_capacity, uint64_t n_texts);
int acm_gpu_chains_records_device (ACMPlan *plan, const ACMChains *chains, const ACMRecord *d_records,
                                   uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                   uint64_t n_symbols, uint64_t pos_base,
                                   const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                   ACMRecord *d_out, uint64_t out_capacity, uint64_t *d_count,
                                   void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_chains_tmp_bytes (const ACMPlan *plan, const ACMChains *chains, uint64_t capacity,
                                      uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_chains_device (ACMPlan *plan, const ACMChains *chains, const void *d_text, uint64_t n_symbols,
                                uint64_t pos_base, const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                uint64_t capacity, ACMRecord *d_out, uint64_t out_capacity,
                                uint64_t *d_count, uint64_t *d_found, void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_chains_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                              const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                              const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains,
                              ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);   /* blocking */
int acm_scan_chains (ACMachine *machine, const void *text, uint64_t n_symbols,
                     const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                     const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains,
                     ACMRecord *out, uint64_t out_capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ keyword templates with symbol classes
 * In PATTERNS and APPROX a position is one exact symbol or anything at all.  TEMPLATES adds "one of these
 * symbols": hex signatures with nibble wildcards and byte ranges (E2 3? ?? [C0-CF] A1), primers in IUPAC
 * codes under a mismatch budget, fixed-column templates such as \d{3}-\d{2}-\d{4}.  It is APPROX with an
 * acceptance test per position that is a set membership: the literal stretches of a template give the
 * pieces, every exact piece record is a seed, and the template is verified against the text around it.
 * The scan kernels stay untouched.
 *
 * DEFINITION.  Classes: there are n_classes classes.  Class c is the set of symbols in the inclusive
 * ranges [cls_ptr[c], cls_ptr[c + 1]) of ranges[] (cls_ptr has n_classes + 1 uint64_t entries); a range is
 * two symbols lo, hi of the caller's symbol size, compared as unsigned integers (acm_words_records'
 * convention).  With cls_flags[c] & ACM_TEMPLATE_NEGATED the class is the complement of that set.  A class
 * has at most ACM_TEMPLATE_MAX_RANGES (16) ranges; an empty class is allowed and accepts nothing, negated
 * it accepts everything.  ACM_GPU_E_ARG: a range with lo > hi, more than 16 ranges, a cls_ptr that
 * decreases or does not begin with 0, n_classes >= 0xFFFFFFFE.
 * Templates: template w has L_w cells, cells[spell_off[w] .. spell_off[w + 1]), one uint32_t each:
 *   ACM_TEMPLATE_LITERAL (0xFFFFFFFF): the cell accepts exactly spell_data[spell_off[w] + i];
 *   ACM_TEMPLATE_ANY (0xFFFFFFFE): the cell accepts every symbol;
 *   a class id < n_classes: the cell accepts the symbols of that class.
 * spell_data has an entry for every cell; it is ignored where the cell is not literal.  Template w has a
 * budget k[w] (at most 255) and the terms [tgt_ptr[w], tgt_ptr[w + 1]), ACMPatternTerm reused as in
 * APPROX: keyword keyword_id, `length` symbols long, is the piece at `offset`.  ACM_GPU_E_ARG: everything
 * acm_approx_check refuses, a cell value that is neither of the two constants nor a class id, and a term
 * that covers a cell that is not literal (a piece is an exact keyword: it stands on literal cells only).
 * The arrays travel in one plain struct of host pointers, ACMTemplateSpec.
 * TEMPLATES (R, text, offsets, T).  Template w MATCHES at buffer index S iff
 *   1. some text t has offsets[t] <= S and S + L_w <= offsets[t + 1], and
 *   2. (seed) some term (kid, o, l) of w has the record (pos_base + S + o + l - 1, l, kid) in R, and
 *   3. d = the number of cells i that do not accept text[S + i] is <= k[w]; symbols are taken bitwise in
 *      the caller's size.
 * Each (w, S) that matches gives exactly one ACMRecord (end_pos = pos_base + S + L_w - 1, length = L_w,
 * keyword_id = w) and dist[r] = d, however many terms seed it.  The total order is end_pos ascending, then
 * length descending, then template id ascending.
 * COMPLETENESS.  When the terms of w are k[w] + 1 pairwise disjoint pieces on literal cells, each keyword
 * is spelled as its piece and R is the full record set, condition 2 follows from 1 and 3: at most k cells
 * fail, so at least one piece is intact.  A template with fewer than k + 1 literal cells cannot be seeded
 * completely; the seed condition then removes matches, which is defined and no error in the record passes.
 * THE CANONICAL CUT.  acm_templates_split (cells, L, k, j, &offset, &length): the literal runs of the
 * template are its maximal stretches of literal cells; q is the largest length with sum over runs of
 * floor (run / q) >= k + 1; each run gives floor (run / q) pieces of q cells from its left end on; piece j
 * is the j-th of these, left to right, for j <= k.  ACM_GPU_E_ARG when the template has fewer than k + 1
 * literal cells.  For k = 0 this is the first of the longest literal runs, whole.
 *
 * acm_templates_check (spec, sym_bytes, n_keywords): the argument checks above, no device; every other
 * entry point runs it.  acm_templates_records: the plain sequential TEMPLATES on the host, no device, with
 * acm_approx_records' rules for overflow, for counting only, for dist == NULL and for ACM_GPU_E_ARG.
 * acm_gpu_templates_create compiles a set once and uploads it to the plan's device (ACMTemplates, opaque):
 * APPROX's index over the terms, the cell words, and the classes -- for 1-byte symbols a bitmap of 256
 * bits per class with the negate flag applied, for wider symbols the ranges and the flags.  A plan over
 * comparator classes is refused with ACM_GPU_E_INELIGIBLE; plans that intern 8-byte symbols are taken;
 * the set stays valid after acm_gpu_plan_update.  acm_gpu_templates_info: templates, terms, classes, the
 * keywords that seed a template, the longest L_w, the largest k and the most postings of one keyword.
 * acm_gpu_templates_records_device (dev_templates.h): acm_gpu_approx_records_device's contract, word for
 * word -- arguments, the four outcomes for count and overflow, the rule for records and offsets that break
 * the contract, launches only -- and its passes: the check of d_offsets in a launch of its own, a count
 * pass with one group of 16 lanes per record over tiles (ACM_GPU_TEMPLATES_TILE=<records>: a multiple of
 * 64 from 64 to 1 Mi, default 1,024), a 64-bit exclusive sum, a fill pass that verifies again, and the
 * order pass when the total fits.  Inside the group lane j takes cells j, j + 16, ...: a literal cell
 * compares with the spelling, an ANY cell accepts without loading the text, a class cell of 1-byte symbols
 * tests one bit of the class's bitmap (one 32-bit load of word sym >> 5, from global memory), a class cell
 * of wider symbols walks the class's ranges.  d_tmp must hold acm_gpu_templates_tmp_bytes bytes.
 * acm_gpu_scan_templates_device / _host, acm_scan_templates: as their APPROX counterparts.  On the machine
 * a term whose keyword is not spelled as its piece is ACM_GPU_E_ARG; a machine with another comparator
 * runs the caller loop and the sequential pass -- literal cells compared by the comparator, class cells by
 * value -- and reports ACM_SCAN_PATH_CPU_LOOP.  A missing device stays an error.
 *
 * Out of scope: templates without a literal cell (a class-only scan kernel); variable-length cells;
 * alternatives (AA|BB); classes inside CHAINS' gaps; edits; flows, streams and several GPUs; class plans
 * on the device. */
#define ACM_TEMPLATE_LITERAL 0xFFFFFFFFu
#define ACM_TEMPLATE_ANY 0xFFFFFFFEu
#define ACM_TEMPLATE_NEGATED 1u
#define ACM_TEMPLATE_MAX_RANGES 16u
typedef struct {
  const void *spell_data;
  const uint64_t *spell_off;
  const uint32_t *cells;
  const uint32_t *k;
  const ACMPatternTerm *terms;
  const uint64_t *tgt_ptr;
  uint64_t n_templates;
  const void *ranges;
  const uint64_t *cls_ptr;
  const uint32_t *cls_flags;
  uint64_t n_classes;
} ACMTemplateSpec;
typedef struct ACMTemplates ACMTemplates;
typedef struct {
  uint64_t templates, terms, classes, seed_keywords, longest, max_k, max_postings;
} ACMTemplatesInfo;
int acm_templates_check (const ACMTemplateSpec *spec, uint32_t sym_bytes, uint64_t n_keywords);
int acm_templates_split (const uint32_t *cells, uint64_t L, uint32_t k, uint32_t j, uint64_t *offset, uint64_t *length);
int acm_templates_records (const ACMRecord *records, uint64_t n, const void *text, uint32_t sym_bytes, uint64_t n_symbols,
                           uint64_t pos_base, const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                           const ACMTemplateSpec *spec, uint64_t n_keywords,
                           ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity, uint64_t *n_found);
int acm_gpu_templates_create (ACMPlan *plan, const ACMTemplateSpec *spec, ACMTemplates **out);
void acm_gpu_templates_destroy (ACMTemplates *templates);
int acm_gpu_templates_info (const ACMTemplates *templates, ACMTemplatesInfo *info);
size_t acm_gpu_templates_tmp_bytes (const ACMPlan *plan, const ACMTemplates *templates, uint64_t n_or_capacity,
                                    uint64_t out_capacity, uint64_t n_texts);
int acm_gpu_templates_records_device (ACMPlan *plan, const ACMTemplates *templates, const ACMRecord *d_records,
                                      uint64_t n_or_capacity, const uint64_t *d_n /* may be NULL */,
                                      const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                                      const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                      ACMRecord *d_out, uint32_t *d_dist /* may be NULL */, uint64_t out_capacity,
                                      uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream);
size_t acm_gpu_scan_templates_tmp_bytes (const ACMPlan *plan, const ACMTemplates *templates, uint64_t capacity,
                                         uint64_t out_capacity, uint64_t n_symbols, uint64_t n_texts);
int acm_gpu_scan_templates_device (ACMPlan *plan, const ACMTemplates *templates, const void *d_text, uint64_t n_symbols,
                                   uint64_t pos_base, const uint64_t *d_offsets /* may be NULL */, uint64_t n_texts,
                                   uint64_t capacity, ACMRecord *d_out, uint32_t *d_dist /* may be NULL */,
                                   uint64_t out_capacity, uint64_t *d_count, uint64_t *d_found,
                                   void *d_tmp, size_t tmp_bytes, void *stream);
int acm_gpu_scan_templates_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base,
                                 const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                                 const ACMTemplateSpec *spec,
                                 ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity,
                                 uint64_t *n_found);   /* blocking */
int acm_scan_templates (ACMachine *machine, const void *text, uint64_t n_symbols,
                        const uint64_t *offsets /* may be NULL */, uint64_t n_texts,
                        const ACMTemplateSpec *spec,
                        ACMRecord *out, uint32_t *dist /* may be NULL */, uint64_t out_capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ several GPUs of one node, one process
 * The reference's model for parallel work is one shared read-only machine and one cursor per worker
 * (/root/reference/README.md:364, aho_corasick.h:70: the caller owns the `const ACState *`).  The
 * cursor after any symbol depends on the last lmax symbols only, so a text splits into R contiguous
 * shards that are scanned independently: shard r owns [r N / R, (r + 1) N / R),
 * starts from the root lmax - 1 symbols earlier (rounded down to a 16-byte boundary of the text)
 * and reports the matches that END inside its range.  An ACMMulti holds one plan per distinct
 * device (tables replicated) and one stream per device; shard r runs on devices[r] -- a device may
 * appear several times (shards of one device run one after the other on its stream), so that
 * `devices = {0,0,0,0,0,0,0,0}` exercises on one GPU everything but the peer copies.
 * The one exchange step: every shard's records are put in canonical order where they were found
 * and copied into their place in one buffer on devices[0] -- hipMemcpyPeerAsync from the other
 * devices (xGMI is point-to-point: these are the direct peer-to-root transfers of SURVEY.md 8e, one
 * per link), a device-to-device copy for shards of devices[0] itself.  Shards own increasing
 * position ranges: their concatenation in shard order IS the canonical order of the whole text. */
typedef struct ACMMulti ACMMulti;
int acm_gpu_multi_create (ACMachine *machine, const int *devices, int n_shards, ACMMulti **out);
void acm_gpu_multi_destroy (ACMMulti *multi);
/* [read_begin, own_end) is what shard `shard` of a text of n_symbols reads, [own_begin, own_end) where its matches end */
int acm_gpu_multi_shard_bounds (const ACMMulti *multi, uint64_t n_symbols, int shard, uint64_t *read_begin,
                                uint64_t *own_begin, uint64_t *own_end);
/* Text in host memory: the shards are uploaded to their devices, scanned, ordered, gathered on
 * devices[0] and copied to `records` (canonical order of the whole text).  Blocking.
 * ACM_GPU_E_OVERFLOW with *n_found = the capacity needed when `capacity` is too small. */
int acm_gpu_multi_scan_host (ACMMulti *multi, const void *text, uint64_t n_symbols, ACMRecord *records,
                             uint64_t capacity, uint64_t *n_found);
/* Shards already resident: d_shard_text[r] is a buffer on devices[r] (16-byte aligned) holding the
 * symbols [read_begin_r, own_end_r) of acm_gpu_multi_shard_bounds.  The records of the whole text
 * arrive in canonical order in d_records, a buffer of `capacity` records on devices[0]; *n_found
 * (host) = their number, which may exceed capacity (ACM_GPU_E_OVERFLOW: nothing dropped silently).
 * Blocking. */
int acm_gpu_multi_scan_device (ACMMulti *multi, const void *const *d_shard_text, uint64_t n_symbols,
                               ACMRecord *d_records, uint64_t capacity, uint64_t *n_found);

/* ------------------------------------------------------------------ one process per GPU: the gather over RCCL
 * The reference's model for parallel work is one shared read-only machine and one cursor per worker
 * (README.md:364, aho_corasick.h:70); across PROCESSES that is one process per GPU, each with its
 * own plan of the same dictionary, its shard of the text (acm_gpu_multi_shard_bounds' rule:
 * contiguous ranges, an lmax - 1 halo) and its records from acm_gpu_scan_ordered_device.  The one
 * exchange step -- BASELINE's "final RCCL gather of match records over xGMI" -- is this call: the
 * counts travel by ncclAllGather, every rank's ordered records by ncclSend to `root`, which
 * receives them (ncclRecv, one group) into their places in ONE buffer: shards own increasing
 * position ranges, so rank order IS the canonical order.  Records travel as 8-byte words when the
 * rank's plan says they fit (acm_gpu_wire_bits; `plan` may be NULL: 16 bytes) and are unpacked on
 * the root.  xGMI is point-to-point: these are the direct peer-to-root transfers of SURVEY.md 8e.
 *
 * librccl.so is loaded when the first of these calls is made (dlopen; $ACM_GPU_COMM_LIB names
 * another library with the same entry points -- the tests' loopback transport), so a single-GPU
 * user of libac75_amd.so never loads it.  `nccl_comm` is an ncclComm_t (rccl.h), passed as void *:
 * the caller's own, or one made here -- acm_gpu_comm_unique_id on one rank, its 128 bytes handed to
 * the others by whatever the processes share (a file, a socket, MPI), acm_gpu_comm_init_rank on
 * every rank with its device current.
 * acm_gpu_comm_gather_records: collective over the communicator, every rank calls it with its own
 * records (d_local[0 .. n_local), positions in [pos_lo, pos_lo + span)); on the root d_all takes
 * `capacity` records.  *n_total (host, every rank) = the records of all ranks; more than the
 * root's capacity: ACM_GPU_E_OVERFLOW on every rank, nothing sent.  The counts are exchanged
 * before the call returns (one stream synchronisation); the transfers and the unpacking are
 * queued on `stream`.  `counts` (host, `world` entries, may be NULL) = records per rank. */
typedef struct ACMComm ACMComm;
int acm_gpu_comm_unique_id (void *id_128_bytes);
int acm_gpu_comm_init_rank (const void *id_128_bytes, int rank, int world, void **nccl_comm);
int acm_gpu_comm_free (void *nccl_comm);
int acm_gpu_comm_create (void *nccl_comm, int rank, int world, int root, ACMComm **out);
void acm_gpu_comm_destroy (ACMComm *comm);
int acm_gpu_comm_gather_records (ACMComm *comm, const ACMPlan *plan, const ACMRecord *d_local, uint64_t n_local,
                                 uint64_t pos_lo, uint64_t span, ACMRecord *d_all, uint64_t capacity,
                                 uint64_t *n_total, uint64_t *counts, void *stream);

/* Waits for the plan's device and reports ACM_GPU_E_INTERNAL if a device-side consistency check
 * ever failed during its scans (never expected), else ACM_GPU_OK. */
int acm_gpu_plan_status (ACMPlan *plan);

/* Kernel timing with HIP events recorded on the launch stream around the scan kernel only.
 * Enable, run scans, then read: total milliseconds and number of launches since enabling.
 * Reading synchronises on the recorded events.  enable = 1: every launch; enable = N > 1: every
 * N-th launch -- the three events of a launch cost about 10 us on the stream (a step of 1 GiB
 * against 1,000 keywords takes 282 us without them and 292 with: tools/exp_timing_overhead.py), so
 * a caller that measures throughput and kernel time in the same run samples.  An
 * acm_gpu_plan_update that rebuilds the plan keeps all of it: the switch, the period N, the place
 * in the period and the totals read so far.  It reads the launches sampled so far into the totals
 * first; a HIP error there is the update's return value, and the plan is left as it was. */
int acm_gpu_plan_timing (ACMPlan *plan, int enable);
int acm_gpu_plan_timing_read (ACMPlan *plan, double *total_ms, uint64_t *launches);
/* the same, and beside the scan kernels' time (scan_ms) the time from the start of each scan kernel
 * to the end of what its launch enqueues behind it -- the expansion of parked items / hits into
 * records, or the closing of the holes in a record buffer the scan kernel wrote itself (all_ms) */
int acm_gpu_plan_timing_read_all (ACMPlan *plan, double *scan_ms, double *all_ms, uint64_t *launches);

/* ------------------------------------------------------------------ synthetic workload (bench/test tooling)
 * text[i] = 'a' + sm(i + 42) % 26, one keyword planted per 4096-symbol block.
 * Generates d_text[0 .. n) for global indices [global_begin, global_begin + n); global_begin must
 * be a multiple of 4096.  kw_data/kw_off: the K keywords packed on the DEVICE (symbols of
 * sym_bytes each; kw_off has K + 1 entries).  For sym_bytes == 4 the unplanted symbol is
 * sm(i + 42) % vocab. */
int acm_gpu_synth_text (int device, void *d_text, uint64_t n, uint64_t global_begin, uint32_t sym_bytes,
                        uint32_t vocab, const void *d_kw_data, const uint32_t *d_kw_off, uint32_t n_kw,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif
#include "acm_score.h"
#include "acm_index.h"
#include "acm_near.h"
#include "acm_cooccur.h"
#include "acm_chars.h"
#include "acm_segment.h"
