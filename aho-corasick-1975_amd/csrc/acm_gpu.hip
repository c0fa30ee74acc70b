/*
 * acm_gpu.hip -- the bulk scan (include/acm_gpu.h) for MI355X / gfx950: device plan, launches,
 * streaming, canonical sort and the C ABI; the kernels are in the dev_*.h files included below
 * (one translation unit).
 *
 * What runs on the device is the reference's caller loop (examples/test.c:17-23): per input
 * symbol one automaton step (acm_match -> state_goto, aho_corasick.c:434-448,167-192) and, when
 * the new state has outputs, the walk over the keyword-terminal states of its failure chain
 * (acm_get_match, aho_corasick.c:459-466), one 16-byte record per match.
 *
 * Kernels
 *   dev_dense.h   scan_dense_kernel   byte alphabets, <= 32,768 states: failure-resolved rows of the
 *                                     hot states in LDS, one ds_read_u16 per symbol, continuation
 *                                     items for the rest (config 2: the headline kernel); sticky
 *                                     mode with rows in HBM for bigger dictionaries
 *   dev_gram.h    scan_gram_kernel    byte alphabets, big dictionaries of keywords >= 4 symbols:
 *                                     4-gram bit table in LDS, every position tested on its own
 *   dev_starts.h  scan_starts_kernel  2- and 4-byte symbols: root table by symbol value in LDS,
 *                                     every position tested on its own; walk_starts, hit parking
 *   dev_sparse.h  scan_sparse_kernel  2- and 4-byte symbols, automaton walk (ACM_GPU_SPARSE=walk)
 *   dev_csr.h     scan_csr_kernel     any width and alignment: goto/failure walk over CSR rows
 *   dev_emit.h    queue items -> records: put_outputs, walk_continuation, flush_queue,
 *                 expand_items_kernel (block-wide prefix sum, one atomic per round)
 *   dev_misc.h    classmap (comparator classes), patch (incremental updates), sort keys, synthetic text
 *   dev_order.h   canonical order by position buckets + LDS sorts (three passes instead of a radix sort's eight)
 * No MFMA anywhere: this is byte/integer table walking bound by LDS lookups and HBM reads.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "acm_internal.h"

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      fprintf (stderr, "acm_gpu: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString (_e), __FILE__, \
               __LINE__);                                                                          \
      return ACM_GPU_E_HIP;                                                                        \
    }                                                                                              \
  } while (0)

/* the host-buffer conveniences: out of memory is told apart; their device buffers belong to a
 * DeviceTemps, so nothing is freed here */
#define HOST_TRY(expr)                                                                             \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      fprintf (stderr, "acm_gpu: %s failed: %s\n", #expr, hipGetErrorString (_e));                  \
      return _e == hipErrorOutOfMemory ? ACM_GPU_E_NOMEM : ACM_GPU_E_HIP;                          \
    }                                                                                              \
  } while (0)

#include "dev_all.h"

/* ====================================================================== host side */
/* Host mirror of the start-parallel tables of a plan that takes incremental updates
 * (acm_gpu_plan_update).  The start-parallel kernel walks the goto function only -- no failure
 * links, no output counts -- so a new keyword touches just the states on its own path: the new
 * ones are appended (ids in order of creation after the breadth-first ids of the plan's build),
 * the state they hang off gets one more edge, and the root table / pair table entries of at most
 * two symbols change.  The changed words are collected as patches and written by patch_kernel on
 * the stream of the next scan, in front of it. */
enum { PT_REC = 0, PT_EDGE = 1, PT_LUT = 2, PT_PAIRS = 3, PT_OINFO = 4 };
struct StartsMirror {
  std::vector<uint32_t> tab[5];           /* rec: 8 per state, edge: 2 per slot, lut, pairs: 2 per state, oinfo: 4 per state */
  std::vector<uint32_t> parent, parent_sym, depth; /* host only, per state */
  uint32_t *dev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
  size_t cap[5] = { 0, 0, 0, 0, 0 };      /* device capacity in words */
  bool own = false;                       /* device arrays of their own (else still inside the plan's blob) */
  bool full_upload = false;
  std::vector<uint4> patches;
  uint4 *d_patches = nullptr;
  size_t cap_patches = 0;
  uint32_t n_states = 0, lmax = 0, n_keywords = 0, n_edges = 0;

  void
  set (int t, size_t idx, uint32_t v) {
    if (idx >= tab[t].size ())
      tab[t].resize (idx + 1, 0);
    if (tab[t][idx] == v)
      return;
    tab[t][idx] = v;
    if (idx >= cap[t] || !own)
      full_upload = true; /* beyond what the device holds (or still in the blob): everything goes up again */
    else if (!full_upload)
      patches.push_back (make_uint4 ((uint32_t)t, (uint32_t)idx, v, 0));
  }
};

/* the kernel family of a plan (ACMPlanInfo::kernel) */
enum class PlanKind : uint32_t { Dense = 1, Csr = 2, Sparse = 3, Starts = 4, Gram = 5 };

/* item buffer of the kernels that park items (dense, start-parallel, 4-gram over hashed windows):
 * regions x region_items items of 8 B, one region per wave.  A plan owns one; its delta parks in
 * the same one (ACMPlan::items). */
struct ItemBuffer {
  void *items = nullptr;
  uint32_t *fill = nullptr; /* per region, zero between launches */
  uint32_t regions = 0, region_items = 0;
};

/* what a scan of the plan writes on the device besides the caller's records: grown on demand, one
 * scan at a time per plan (a delta has its own) */
struct ScanScratch {
  unsigned long long *d_total = nullptr; /* [0] running total of a scan, [1] low word = expand ticket; zero between scans */
  unsigned int *d_pool_ctr = nullptr;    /* 2 x POOL_CLASSES tile-pool counters (same allocation), alternating per launch */
  uint32_t launch_seq = 0;
  /* the text the kernels walk when it is not the caller's: class ids, interned ids, an aligned copy */
  void *d_remap = nullptr;
  size_t remap_bytes = 0;
  /* 4-gram kernel, narrow alphabets (records straight from the scan kernel): one hole descriptor
   * per wave and the spill area, one chunk of records per wave (64 MB on 256 CUs) */
  void *d_holes = nullptr, *d_spill = nullptr;
  uint32_t spill_chunk = 0; /* slots per chunk the spill area was sized for */
  uint32_t direct_regions = 0;
};

struct ACMPlan {
  /* ---- tables and facts fixed when the plan is built (incremental updates of a Starts plan edit
   * finfo, TK and d_oinfo: acm_gpu_plan_update, starts_flush) */
  int device = 0;
  PlanKind kind = PlanKind::Csr;
  ACMFlatInfo finfo{};
  ACMPlanInfo info{};
  void *blob = nullptr; /* one device allocation holding every table */
  size_t blob_bytes = 0;
  int cu_count = 0;
  uint64_t segment = SEGMENT;
  /* CSR kernel (breadth-first numbering) */
  CsrTables csr{};
  const uint4 *d_oinfo = nullptr;
  const uint32_t *d_kw4 = nullptr;
  const uint16_t *d_cont_dh = nullptr;
  const uint4 *d_chain = nullptr; /* EmitCtx::chain */
  /* sparse kernel (2- and 4-byte symbols) */
  SparseK SK{};  /* Sparse and Starts plans (Starts: segments that are not 16-byte aligned) */
  StartsK TK{};
  StartsMirror *mir = nullptr; /* Starts plans: what acm_gpu_plan_update edits */
  GramK GK{};
  /* Gram plans, two forms by alphabet:
   *   narrow (!hashed: up to 29 symbols + "other"): exact base-W 4-gram index, records written by the
   *     scan kernel itself; gram2: scan_gram2_kernel (dev_gram2.h) instead of scan_gram_kernel (up to
   *     26 symbols + "other"); short_pass: the keywords of 1-3 symbols in a pass of their own
   *     (scan_short_kernel, dev_short.h), short_ids_lds: that pass has their ids in LDS;
   *   hashed: hashed 4-byte windows, hits parked and expanded; inline_shorts: the keywords of 1-3
   *     symbols in the kernel's own third queue.
   * So gram2 and short_pass (with short_ids_lds) only with !hashed, inline_shorts only with hashed. */
  bool hashed = false, gram2 = false, short_pass = false, short_ids_lds = false, inline_shorts = false;
  uint32_t short_lds_bytes = 0, short_lds_count_bytes = 0; /* scan_short_kernel: with records / count-only (the nibbles alone) */
  uint32_t short_blocks_per_cu = 1; /* scan_short_kernel, count-only: two blocks a CU when its LDS allows (8 waves a SIMD) */
  uint32_t gram_lds_bytes = 0;
  uint32_t class_sym_bytes = 0; /* comparator-class plans: the symbol size they were made for */
  bool sparse_lut_lds = false, starts_lut_lds = false;
  uint32_t sparse_lds_bytes = 0, starts_lds_bytes = 0;
  /* dense kernel (breadth-first numbering too: the LDS rows are a breadth-first prefix) */
  DenseK K{};
  const void *d_dense = nullptr;     /* failure-resolved rows of every state */
  const void *d_lds_image = nullptr; /* what every workgroup copies into LDS */
  const uint32_t *d_wrows = nullptr;
  const uint32_t *d_dstart = nullptr;
  uint32_t lds_image_bytes = 0;
  /* dynamic LDS of a launch: info.lds_bytes (what the rows, hotfail, queues and tile counter
   * occupy) in sticky mode, DENSE_HF_END in continuation mode (the unused gap included) */
  uint32_t dense_lds_launch = 0;
  uint32_t entry_bytes = 0, streams = ACM_DENSE_S, chunk = 64;
  /* comparator-class plans: the text is mapped to class ids into scratch.d_remap before every scan */
  uint16_t *d_classlut = nullptr;
  /* 8-byte symbols: hash table {key, id} of the dictionary's symbols; the text is interned to
   * 4-byte ids into scratch.d_remap and finfo.sym_bytes is 4 (what the kernels walk) */
  uint4 *d_intern = nullptr;
  uint32_t intern_mask = 0;
  uint32_t text_sym_bytes = 0; /* symbol size of the caller's text (== finfo.sym_bytes unless interned) */
  /* comparator classes of 4-byte symbols (ACMFlatView::keys32): every symbol classified so far ->
   * class, on the host and as the device's table {symbol, class + 1}; the text is mapped to class
   * ids into scratch.d_remap before every scan and symbols met for the first time are classified on
   * the host with the machine's comparator (cmp32; classify_text32) -- so these grow with the texts */
  bool cls32 = false;
  std::unordered_map<uint32_t, uint32_t> cls32_known;
  std::vector<uint32_t> cls32_reps; /* one symbol per class, comparator order: class i + 1 */
  CMP_TYPE cmp32 = nullptr;
  void *cmp32_arg = nullptr;
  unsigned long long *d_cls32 = nullptr;
  uint32_t cls32_slots = 0, cls32_uploaded = 0; /* table size; known symbols it holds */
  uint32_t *d_unknown = nullptr; /* [0] count, [1 .. cls32_cap] symbols */
  /* symbols one pass can hand to the host: doubled (up to CLS32_CAP_MAX) whenever a pass fills the
   * list, so that a text of many distinct symbols takes a few passes, not one per 65,536 of them;
   * the plan refuses texts that bring more than CLS32_KNOWN_MAX distinct symbols in all (the host
   * map and the device table hold every one of them) */
  static constexpr uint32_t CLS32_CAP_MIN = 1u << 16, CLS32_CAP_MAX = 1u << 22, CLS32_KNOWN_MAX = 1u << 25;
  uint32_t cls32_cap = CLS32_CAP_MIN;

  /* ---- what a scan writes */
  ItemBuffer own_items;
  ItemBuffer *shared_items = nullptr; /* delta plans: the buffer of the plan they belong to (scans of the two never overlap) */
  ItemBuffer &items () { return shared_items ? *shared_items : own_items; }
  ScanScratch scratch;

  /* ---- update state (acm_gpu_plan_update; scan_plan counts delta_scanned and marks `retired`) */
  uint64_t generation = 0; /* for the machine-cached plan */
  /* Dictionary growth without a rebuild (acm_gpu_plan_update): the keywords a machine got after
   * this plan was made live in a small second plan, `delta`, scanned right after this one into the
   * same record buffer (the match set of a dictionary is the union of its keywords' match sets;
   * the delta's keyword ids start at kw_base).  A replaced delta waits in `retired` until the
   * stream that may still be scanning with it has passed an event. */
  ACMPlan *delta = nullptr;
  uint64_t delta_scanned = 0;    /* symbols scanned twice (plan, then delta) since this delta's first keyword came */
  uint32_t covered_keywords = 0; /* keywords of the machine this plan and its delta report */
  uint32_t kw_base = 0;          /* added to the keyword ids of this plan's records (delta plans) */
  uint32_t merges = 0;           /* updates that rebuilt everything */
  struct Retired {
    ACMPlan *plan;
    hipEvent_t done; /* nullptr until the first scan after the retirement has recorded it */
  };
  std::vector<Retired> retired;

  /* ---- timing state (acm_gpu_plan_timing*, timing_begin) */
  bool timing = false;
  uint32_t timing_every = 1, timing_seq = 0; /* events around every timing_every-th launch (acm_gpu_plan_timing) */
  struct LaunchEvents {
    hipEvent_t start, scan_done, all_done; /* around the scan kernel; after what follows it (expansion / hole closing) */
  };
  std::vector<LaunchEvents> events;
  size_t events_used = 0;
  double timing_ms = 0, timing_all_ms = 0;
  uint64_t timing_launches = 0;
};

extern "C" const char *
acm_gpu_strerror (int code) {
  switch (code) {
  case ACM_GPU_OK: return "ok";
  case ACM_GPU_E_INELIGIBLE: return "machine not eligible for the GPU path (needs ACM_CMP_DEFAULT over 1/2/4-byte symbols)";
  case ACM_GPU_E_NODEVICE: return "no usable HIP device";
  case ACM_GPU_E_HIP: return "HIP runtime error";
  case ACM_GPU_E_OVERFLOW: return "record buffer too small";
  case ACM_GPU_E_ARG: return "invalid argument";
  case ACM_GPU_E_NOMEM: return "out of memory";
  case ACM_GPU_E_INTERNAL: return "internal consistency check failed on the device";
  case ACM_GPU_E_FORMAT: return "not a valid flat-table blob";
  case ACM_GPU_E_IO: return "file could not be read or written";
  case ACM_GPU_E_COMM: return "librccl.so could not be loaded or an RCCL call failed";
  default: return "unknown error";
  }
}

extern "C" int
acm_gpu_device_count (void) {
  int n = 0;
  if (hipGetDeviceCount (&n) != hipSuccess)
    return 0;
  return n;
}

namespace {

size_t
blob_reserve (size_t &cursor, size_t bytes) {
  cursor = (cursor + 255) & ~(size_t)255;
  size_t at = cursor;
  cursor += bytes;
  return at;
}

/* ---- the compiled sets (rules, score, patterns, chains, approx): one allocation on the plan's device.
 * What every set begins with ... */
struct DeviceSet {
  int device = 0;
  void *blob = nullptr; /* one allocation: the set's arrays */
  uint32_t n_keywords = 0;
};

/* ... how its blob is made: the parts are added as (what to copy or NULL, bytes to copy, bytes to reserve) under
 * blob_reserve's 256-byte rule, upload () allocates once, clears the whole blob (the form counters of rules and
 * score begin at 0) and copies part by part, and at<T> () is a part's place -- never NULL, also for no bytes ... */
struct BlobBuilder {
  struct Part {
    const void *from;
    size_t copy, at;
  };
  std::vector<Part> parts;
  size_t bytes = 0;
  unsigned char *base = nullptr;
  size_t
  add (const void *from, size_t copy, size_t reserve) {
    parts.push_back (Part{ from, copy, blob_reserve (bytes, reserve) });
    return parts.size () - 1;
  }
  size_t
  add (const void *from, size_t copy) {
    return add (from, copy, copy);
  }
  bool
  upload (void **blob) {
    if (hipMalloc (blob, bytes) != hipSuccess || hipMemset (*blob, 0, bytes) != hipSuccess)
      return false;
    base = static_cast<unsigned char *> (*blob);
    for (const Part &p : parts)
      if (p.copy && hipMemcpy (base + p.at, p.from, p.copy, hipMemcpyHostToDevice) != hipSuccess)
        return false;
    return hipDeviceSynchronize () == hipSuccess;
  }
  template <typename T = void>
  T *
  at (size_t part) const {
    return reinterpret_cast<T *> (base + parts[part].at);
  }
};

/* ... and how it goes away (the body of the five acm_gpu_*_destroy) */
template <typename Set>
void
set_destroy (Set *set) {
  if (!set)
    return;
  (void)hipSetDevice (set->device);
  if (set->blob)
    (void)hipFree (set->blob);
  delete set;
}

/* the blob of a new set on the device, or ACM_GPU_E_NOMEM and the half-made set destroyed */
template <typename Set>
int
set_upload (Set *set, BlobBuilder &b) {
  if (b.upload (&set->blob))
    return ACM_GPU_OK;
  set_destroy (set);
  return ACM_GPU_E_NOMEM;
}

int
env_int (const char *name, int absent) {
  const char *e = getenv (name);
  return e ? atoi (e) : absent;
}

/* the plan's error flag (acm_gpu_plan_status reads it), nullptr while the plan has no scratch */
unsigned int *
error_word (const ACMPlan *plan) {
  return plan->scratch.d_total ? reinterpret_cast<unsigned int *> (plan->scratch.d_total) + 3 : nullptr;
}

/* grid of a grid-stride kernel: `blocks`, at least one, never more than per_cu a CU */
dim3
capped_grid (const ACMPlan *plan, uint64_t blocks, uint32_t per_cu = 8) {
  const uint64_t most = (uint64_t)plan->cu_count * per_cu;
  return dim3 ((uint32_t)(blocks < 1 ? 1 : blocks < most ? blocks : most));
}

/* scratch of hipcub's exclusive sum over n 32-bit counts */
size_t
exclusive_sum_bytes (uint64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum (nullptr, bytes, static_cast<uint32_t *> (nullptr), static_cast<uint32_t *> (nullptr), (int)n, nullptr);
  return bytes;
}

/* the same over n signed 64-bit sums */
size_t
exclusive_sum_bytes64 (uint64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum (nullptr, bytes, static_cast<long long *> (nullptr), static_cast<long long *> (nullptr), (int)n, nullptr);
  return bytes;
}

/* the longest keyword of the plan and of its delta.  acm_gpu_plan_update keeps plan->finfo.lmax at
 * the maximum of both ("halos and sort keys go by the longest keyword of both"), so this equals
 * plan->finfo.lmax; the form says what is meant */
uint32_t
plan_lmax (const ACMPlan *plan) {
  const uint32_t own = plan->finfo.lmax, more = plan->delta ? plan->delta->finfo.lmax : 0;
  return own > more ? own : more;
}

/* bits of a sort key's length field: every length in [0, lmax] */
uint32_t
len_bits_of (uint32_t lmax) {
  uint32_t bits = 1;
  while ((1u << bits) <= lmax)
    bits++;
  return bits;
}

/* temporary device memory of one call: blocks of at least 16 bytes, freed when the call returns */
struct DeviceTemps {
  std::vector<void *> blocks;
  DeviceTemps () = default;
  DeviceTemps (const DeviceTemps &) = delete;
  DeviceTemps &operator= (const DeviceTemps &) = delete;
  ~DeviceTemps () {
    for (void *b : blocks)
      (void)hipFree (b);
  }
  template <typename T>
  hipError_t
  get (T **out, size_t bytes) {
    void *b = nullptr;
    const hipError_t e = hipMalloc (&b, bytes < 16 ? 16 : bytes);
    if (e == hipSuccess)
      blocks.push_back (b);
    *out = static_cast<T *> (b);
    return e;
  }
  hipError_t
  release (void *b) { /* one block before the others */
    blocks.erase (std::remove (blocks.begin (), blocks.end (), b), blocks.end ());
    return hipFree (b);
  }
};

/* ---- what the device entry points share.
 * The scratch of one call, taken buffer by buffer from `d_tmp` under blob_reserve's 256-byte rule.
 * Without a base nothing is bound (take () gives nullptr) and only the size is kept: a family's
 * *_carve function runs once without a base for *_tmp_bytes and once over d_tmp for the device
 * call, so what is reported and what is bound are the same lines. */
struct Carve {
  uintptr_t base;
  size_t used = 0;
  explicit Carve (void *d_tmp = nullptr) : base (reinterpret_cast<uintptr_t> (d_tmp)) {}
  template <typename T = unsigned char>
  T *
  take (size_t count) {
    const size_t at = blob_reserve (used, count * sizeof (T));
    return base ? reinterpret_cast<T *> (base + at) : nullptr;
  }
  size_t
  boundary () { /* where the next buffer will begin */
    return blob_reserve (used, 0);
  }
  size_t
  total () const { /* what *_tmp_bytes reports */
    return used + 256;
  }
};

/* hipcub's scratch inside a carve: room for the exclusive sum over n32 32-bit counts and over n64
 * 64-bit sums, whichever needs more */
struct CubRoom {
  void *at = nullptr;
  size_t bytes = 0;
};
CubRoom
cub_room (Carve &c, uint64_t n32, uint64_t n64) {
  CubRoom r;
  r.bytes = std::max (n32 ? exclusive_sum_bytes (n32) : 0, n64 ? exclusive_sum_bytes64 (n64) : 0);
  r.at = c.take (r.bytes + 16);
  return r;
}

/* out[i] = in[0] + ... + in[i - 1] over n items of either width, queued on st */
template <typename In, typename Out>
hipError_t
exclusive_sum (const CubRoom &cub, In in, Out out, uint64_t n, hipStream_t st) {
  size_t bytes = cub.bytes;
  return hipcub::DeviceScan::ExclusiveSum (cub.at, bytes, in, out, (int)n, st);
}

/* a kernel launch and what it left: HIP_TRY (launch (...)) */
template <typename... Params, typename... Args>
hipError_t
launch (void (*kernel) (Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
  hipLaunchKernelGGL (kernel, grid, block, lds, st, args...);
  return hipGetLastError ();
}

/* a test tunable, read from the environment at every call: `absent` unless the value lies in
 * [lo, hi] and keeps the rule */
enum class Tune { Any, Mult16, MultWave, Pow2 };
uint32_t
tunable (const char *name, uint32_t absent, uint32_t lo, uint32_t hi, Tune rule) {
  const int v = env_int (name, (int)absent);
  const bool fits = v >= (int)lo && v <= (int)hi &&
                    (rule == Tune::Any || (rule == Tune::Mult16 && v % 16 == 0) || (rule == Tune::MultWave && v % (int)WAVE == 0) ||
                     (rule == Tune::Pow2 && (v & (v - 1)) == 0));
  return fits ? (uint32_t)v : absent;
}

/* ---- the kernel a plan launches, by the plan's own facts: set_lds_attributes and the launch
 * functions ask the same function, so the attribute is set on what is launched */
#define KERNEL_FN(...) reinterpret_cast<const void *> (&__VA_ARGS__)
/* one geometry is built: 64-byte chunks, 2 streams per lane (the template takes others) */
const void *
dense_kernel (const ACMPlan *p, bool count_only) {
  if (p->entry_bytes == 2)
    return count_only ? KERNEL_FN (scan_dense_kernel<uint16_t, 64, ACM_DENSE_S, true>) : KERNEL_FN (scan_dense_kernel<uint16_t, 64, ACM_DENSE_S, false>);
  return count_only ? KERNEL_FN (scan_dense_kernel<uint32_t, 64, ACM_DENSE_S, true>) : KERNEL_FN (scan_dense_kernel<uint32_t, 64, ACM_DENSE_S, false>);
}

template <typename SYM>
const void *
sparse_fn (bool lut_lds, bool count_only) {
  if (lut_lds)
    return count_only ? KERNEL_FN (scan_sparse_kernel<SYM, true, true>) : KERNEL_FN (scan_sparse_kernel<SYM, true, false>);
  return count_only ? KERNEL_FN (scan_sparse_kernel<SYM, false, true>) : KERNEL_FN (scan_sparse_kernel<SYM, false, false>);
}

const void *
sparse_kernel (const ACMPlan *p, bool count_only) {
  return p->finfo.sym_bytes == 2 ? sparse_fn<uint16_t> (p->sparse_lut_lds, count_only) : sparse_fn<uint32_t> (p->sparse_lut_lds, count_only);
}

template <typename SYM>
const void *
starts_fn (bool lut_lds, bool count_only) {
  if (lut_lds)
    return count_only ? KERNEL_FN (scan_starts_kernel<SYM, true, true>) : KERNEL_FN (scan_starts_kernel<SYM, true, false>);
  return count_only ? KERNEL_FN (scan_starts_kernel<SYM, false, true>) : KERNEL_FN (scan_starts_kernel<SYM, false, false>);
}

const void *
short_kernel (const ACMPlan *p, bool count_only) {
  if (count_only)
    return KERNEL_FN (scan_short_kernel<true, true>);
  return p->short_ids_lds ? KERNEL_FN (scan_short_kernel<false, true>) : KERNEL_FN (scan_short_kernel<false, false>);
}

/* tiled: a tiled scan (narrow alphabets, record mode) */
const void *
gram_kernel (const ACMPlan *p, bool count_only, bool tiled) {
  const bool wide = p->hashed, shorts = p->inline_shorts;
  if (p->gram2) {
    if (tiled)
      return KERNEL_FN (scan_gram2_kernel<false, true>);
    return count_only ? KERNEL_FN (scan_gram2_kernel<true, false>) : KERNEL_FN (scan_gram2_kernel<false, false>);
  }
  /* (keywords of 1-3 symbols inside the kernel: hashed windows only -- narrow alphabets give them a
   * pass of their own, scan_short_kernel; the instantiations that did both spilled 140 to 320 vector registers) */
  if (tiled) /* (narrow alphabets, record mode) */
    return KERNEL_FN (scan_gram_kernel<false, false, false, true>);
  if (wide && shorts)
    return count_only ? KERNEL_FN (scan_gram_kernel<true, true, true, false>) : KERNEL_FN (scan_gram_kernel<false, true, true, false>);
  if (wide)
    return count_only ? KERNEL_FN (scan_gram_kernel<true, false, true, false>) : KERNEL_FN (scan_gram_kernel<false, false, true, false>);
  return count_only ? KERNEL_FN (scan_gram_kernel<true, false, false, false>) : KERNEL_FN (scan_gram_kernel<false, false, false, false>);
}

const void *
starts_kernel (const ACMPlan *p, bool count_only) {
  return p->finfo.sym_bytes == 2 ? starts_fn<uint16_t> (p->starts_lut_lds, count_only) : starts_fn<uint32_t> (p->starts_lut_lds, count_only);
}
#undef KERNEL_FN

void
drop_cached_plan (void *p) {
  acm_gpu_plan_destroy (static_cast<ACMPlan *> (p));
}

} // namespace

namespace {
/* ---- table builders of acm_gpu_plan_create_flat (host images of the device tables) */

/* sparse automaton walk (dev_sparse.h): state records, (symbol, next | out flag) edges, root table */
void
fill_sparse_tables (const ACMFlatView &fv, const ACMFlatInfo &fi, uint32_t lut_size, uint32_t *rec, uint32_t *edge, uint32_t *lut) {
  const uint32_t n = fi.n_states;
  auto entry = [&] (uint32_t e) { return fv.edge_next[e] | (fv.nb_outputs[fv.edge_next[e]] ? 0x80000000u : 0u); };
  for (uint32_t e = 0; e < fi.n_edges; e++) {
    edge[2 * e] = fv.edge_sym[e];
    edge[2 * e + 1] = entry (e);
  }
  for (uint32_t st = 0; st < n; st++) {
    const uint32_t b = fv.row_ptr[st], ne = fv.row_ptr[st + 1] - b;
    uint32_t *r = rec + 8 * (size_t)st;
    r[0] = fv.fail[st];
    r[1] = ne;
    r[2] = b;
    r[3] = 0;
    r[4] = ne >= 1 ? fv.edge_sym[b] : 0;
    r[5] = ne >= 1 ? entry (b) : 0;
    r[6] = ne >= 2 ? fv.edge_sym[b + 1] : 0;
    r[7] = ne >= 2 ? entry (b + 1) : 0;
  }
  for (uint32_t e = 0; e < fv.row_ptr[1]; e++)
    if (fv.edge_sym[e] < lut_size)
      lut[fv.edge_sym[e]] = entry (e);
}

/* start-parallel kernel (dev_starts.h): trie records with terminal flags, plain edges, root table
 * with SECOND / ALWAYS flags, first-two-edge-symbols of the root's children */
void
fill_starts_tables (const ACMFlatView &fv, const ACMFlatInfo &fi, uint32_t lut_size, uint32_t *rec, uint32_t *edge, uint32_t *lut,
                    uint32_t *pairs) {
  const uint32_t n = fi.n_states;
  for (uint32_t e = 0; e < fi.n_edges; e++) {
    edge[2 * e] = fv.edge_sym[e];
    edge[2 * e + 1] = fv.edge_next[e];
  }
  for (uint32_t st = 0; st < n; st++) {
    const uint32_t b = fv.row_ptr[st], ne = fv.row_ptr[st + 1] - b;
    uint32_t *r = rec + 8 * (size_t)st;
    r[0] = 0;
    r[1] = ne;
    r[2] = b;
    r[3] = fv.term_kw[st] != NONE ? 1u : 0u;
    r[4] = ne >= 1 ? fv.edge_sym[b] : 0;
    r[5] = ne >= 1 ? fv.edge_next[b] : 0;
    r[6] = ne >= 2 ? fv.edge_sym[b + 1] : 0;
    r[7] = ne >= 2 ? fv.edge_next[b + 1] : 0;
  }
  const uint32_t root_edges = fv.row_ptr[1];
  {
    /* the root's row in the edge table: only the symbols the root table cannot hold (the tail
     * of the sorted row; usually nothing) -- the table itself answers for the others */
    uint32_t beyond = 0;
    while (beyond < root_edges && fv.edge_sym[root_edges - 1 - beyond] >= lut_size)
      beyond++;
    rec[1] = beyond;
    rec[2] = root_edges - beyond;
  }
  for (uint32_t st = 0; st <= root_edges; st++) {
    const uint32_t b = fv.row_ptr[st], ne = fv.row_ptr[st + 1] - b;
    pairs[2 * st] = ne >= 1 ? fv.edge_sym[b] : 0;
    pairs[2 * st + 1] = ne >= 2 ? fv.edge_sym[b + 1] : pairs[2 * st];
  }
  for (uint32_t e = 0; e < root_edges; e++)
    if (fv.edge_sym[e] < lut_size) {
      const uint32_t child = fv.edge_next[e];
      const uint32_t ne = fv.row_ptr[child + 1] - fv.row_ptr[child];
      /* keyword by itself, more edges than the pair shows, or a pair that cannot be told
       * from "no edge" (symbol 0 twice): never sieved out */
      const bool always = fv.term_kw[child] != NONE || ne > 2 || ne == 0;
      lut[fv.edge_sym[e]] = child | (always ? ST_ALWAYS : 0u);
    }
  /* second symbols: the edges that leave the root's children (states 1 .. root_edges) */
  for (uint32_t e = fv.row_ptr[1]; e < fv.row_ptr[root_edges + 1]; e++)
    if (fv.edge_sym[e] < lut_size)
      lut[fv.edge_sym[e]] |= ST_SECOND;
}

/* 4-gram sieve kernel (dev_gram.h): where its tables go and how they are keyed */
struct GramImage {
  bool wide, shorts;
  uint32_t W, bloom_log2, wtab_log2, stab_log2;
  uint32_t *bits, *g4, *rec, *edge, *g4gid; /* first-stage bits, second-stage records, trie records (depth-first), their edges, depth-4 state -> record */
  unsigned char *nib;                      /* narrow alphabets: nibble per 3-gram */
  uint32_t *prefix, *entry;                /* narrow alphabets: set bits before each word of `bits`; by rank {children mask | terminal << 31, first child's state id, keyword id} */
  uint32_t *peek;                          /* narrow alphabets: per depth-5 state {its record, the symbol of its only edge or GRAM_NO_PEEK} */
  uint32_t *bloom;                         /* narrow alphabets: Bloom bits, terminal 4-grams then 5-grams (GramK::bloom5_bits; NULL: none) */
  uint32_t bloomT_bits, bloom5_bits, lo, kw_base;
  bool kw_inline;                          /* keyword ids fit a hit's word (HIT_KW) */
  bool peek_packed;                        /* 4 bytes per depth-5 state (fewer than 2^23 records) instead of 8 */
  uint32_t *g3, *stab;                     /* short keywords: prefix states per 3-gram (narrow) / table of tagged windows (wide) */
  uint32_t *tab2;                          /* scan_gram2_kernel: two bits per 4-gram (GramK::tab2); NULL: not made */
  uint32_t *rows2, *over2;                 /* the second stage's entries by row of 16 4-grams (GramK::rows2), the rows' 8th and later entries */
};

void
fill_gram_tables (const ACMFlatView &fv, const ACMFlatInfo &fi, const GramImage &G) {
  const uint32_t n = fi.n_states;
  uint32_t *bits = G.bits, *g4 = G.g4, *rec = G.rec, *edge = G.edge, *g4gid = G.g4gid;
  {
    /* records of the states of depth >= 4 in depth-first (preorder) order, subtree after
     * subtree of the depth-4 states: the tail of a keyword is a run of consecutive 32-byte
     * records, so a walk touches one or two cache lines instead of one per symbol */
    std::vector<uint32_t> gid (n, 0), stack;
    uint32_t next_gid = 0;
    for (uint32_t root4 = fv.depth_start[4]; root4 < fv.depth_start[5]; root4++) {
      g4gid[root4 - fv.depth_start[4]] = next_gid;
      stack.push_back (root4);
      while (!stack.empty ()) {
        const uint32_t st = stack.back ();
        stack.pop_back ();
        gid[st] = next_gid++;
        for (uint32_t e = fv.row_ptr[st + 1]; e-- > fv.row_ptr[st];) /* first child on top */
          stack.push_back (fv.edge_next[e]);
      }
    }
    uint32_t slots = 0;
    for (uint32_t st = fv.depth_start[4]; st < n; st++) {
      const uint32_t b0 = fv.row_ptr[st], ne = fv.row_ptr[st + 1] - b0;
      uint32_t *r = rec + 8 * (size_t)gid[st];
      r[0] = st;
      r[1] = ne | (fv.depth[st] << 16); /* (byte alphabet: at most 256 edges; depth < 4,096: the dense eligibility test) */
      r[2] = slots;
      r[3] = fv.term_kw[st] != NONE ? fv.term_kw[st] + G.kw_base + 1u : 0u; /* terminal: keyword id + 1 (a record written on the spot needs it) */
      r[4] = ne >= 1 ? fv.edge_sym[b0] : 0;
      r[5] = ne >= 1 ? gid[fv.edge_next[b0]] : 0;
      r[6] = ne >= 2 ? fv.edge_sym[b0 + 1] : 0;
      r[7] = ne >= 2 ? gid[fv.edge_next[b0 + 1]] : 0;
      for (uint32_t e = b0; e < b0 + ne; e++) {
        edge[2 * (size_t)slots] = fv.edge_sym[e];
        edge[2 * (size_t)slots + 1] = gid[fv.edge_next[e]];
        slots++;
      }
    }
    /* what a walk that starts at a depth-5 state asks first (GramK::g5peek): where its record is,
     * and -- when the state is no keyword's end and has one way on -- the symbol that way takes,
     * so that 25 of 26 candidates end on 8 bytes that stay in L2 instead of a 32-byte record
     * from the 16 MB of them */
    const uint32_t d5_end = fi.lmax >= 5 ? fv.depth_start[6 <= fi.lmax + 1 ? 6 : fi.lmax + 1] : fv.depth_start[5];
    for (uint32_t st = fv.depth_start[5]; G.peek && fi.lmax >= 5 && st < d5_end; st++) {
      const uint32_t b0 = fv.row_ptr[st], ne = fv.row_ptr[st + 1] - b0;
      const uint32_t sym = (ne == 1 && fv.term_kw[st] == NONE) ? fv.edge_sym[b0] : GRAM_NO_PEEK;
      if (G.peek_packed) /* record | symbol << 23 | "look at the record" << 31 */
        G.peek[st - fv.depth_start[5]] = gid[st] | (sym == GRAM_NO_PEEK ? 0x80000000u : sym << 23);
      else {
        G.peek[2 * (size_t)(st - fv.depth_start[5])] = gid[st];
        G.peek[2 * (size_t)(st - fv.depth_start[5]) + 1] = sym;
      }
    }
  }
  /* base-W number of the path of every state down to depth 4 (parents come first in
   * breadth-first order); the depth-4 states are the 4-grams some keyword starts with */
  std::vector<uint32_t> path (fv.depth_start[5 <= fi.lmax + 1 ? 5 : fi.lmax + 1], 0);
  for (uint32_t st = 0; st < fv.depth_start[4]; st++)
    for (uint32_t e = fv.row_ptr[st]; e < fv.row_ptr[st + 1]; e++)
      path[fv.edge_next[e]] = G.wide ? path[st] | (fv.edge_sym[e] << (8 * fv.depth[st])) /* the 4 bytes as the text holds them */
                                        : path[st] * G.W + (fv.edge_sym[e] - fi.alpha_lo);
  for (uint32_t st = fv.depth_start[4]; G.wide && st < fv.depth_start[5]; st++) {
    const uint32_t win = path[st];
    const uint32_t hb = (win * WIDE_H1) >> (32 - G.bloom_log2);
    bits[hb >> 5] |= 1u << (hb & 31);
    uint32_t slot = (win * WIDE_H2) >> (32 - G.wtab_log2);
    while (g4[2 * (size_t)slot + 1])
      slot = (slot + 1) & ((1u << G.wtab_log2) - 1);
    g4[2 * (size_t)slot] = win;
    g4[2 * (size_t)slot + 1] = st | (fv.term_kw[st] != NONE ? WT_TERM : 0u) | (fv.row_ptr[st + 1] > fv.row_ptr[st] ? WT_KIDS : 0u);
  }
  uint32_t n_over2 = 0, row_over = 0;
  std::vector<uint8_t> row_fill (G.rows2 ? (G.W * G.W * G.W * G.W + 15) / 16 : 0, 0); /* (a row has 16 4-grams) */
  for (uint32_t st = fv.depth_start[4]; !G.wide && st < fv.depth_start[5]; st++) {
    const uint32_t idx = path[st];
    uint32_t mask = fv.term_kw[st] != NONE ? 0x80000000u : 0u;
    for (uint32_t e = fv.row_ptr[st]; e < fv.row_ptr[st + 1]; e++)
      mask |= 1u << (fv.edge_sym[e] - fi.alpha_lo);
    bits[idx >> 5] |= 1u << (idx & 31);
    if (G.rows2) {
      /* the entry of this 4-gram: slot r of its row when it is the r-th (< 7) 4-gram of the row that
       * exists (the depth-4 states come in ascending index order), else the next entry of the
       * overflow array, whose first index for the row stands in slot 7 */
      const uint32_t row = idx >> 4;
      const uint32_t r = row_fill[row]++;
      const bool term = fv.term_kw[st] != NONE, kids = fv.row_ptr[st + 1] > fv.row_ptr[st];
      uint32_t e0 = (mask & 0x3FFFFFFFu) | (term ? 0x80000000u : 0u), e1;
      if (term && kids) { /* a keyword of 4 symbols that others go on from: left to the walk, at its own record */
        e0 |= 0x40000000u;
        e1 = g4gid[st - fv.depth_start[4]];
      } else
        e1 = term ? fv.term_kw[st] + G.kw_base : fv.edge_next[fv.row_ptr[st]];
      if (r < 8) { /* (slot 7: the 8th entry itself while there is no 9th) */
        G.rows2[16 * (size_t)row + 2 * r] = e0;
        G.rows2[16 * (size_t)row + 2 * r + 1] = e1;
      }
      if (r >= 7) {
        if (r == 7)
          row_over = n_over2;
        if (r == 8) { /* nine or more: slot 7 says where the 8th and later entries are */
          G.rows2[16 * (size_t)row + 14] = 0x20000000u | row_over;
          G.rows2[16 * (size_t)row + 15] = 0;
        }
        G.over2[2 * (size_t)n_over2] = e0;
        G.over2[2 * (size_t)n_over2 + 1] = e1;
        n_over2++;
      }
    }
    if (G.tab2) {
      /* T of this 4-gram; H of it when it is a keyword; H of the tails of the 5-grams below it */
      const bool term = fv.term_kw[st] != NONE;
      G.tab2[idx >> 4] |= (term ? 3u : 1u) << (2 * (idx & 15));
      const uint32_t W3 = G.W * G.W * G.W;
      for (uint32_t e = fv.row_ptr[st]; e < fv.row_ptr[st + 1]; e++) {
        const uint32_t tail = (idx % W3) * G.W + (fv.edge_sym[e] - fi.alpha_lo);
        G.tab2[tail >> 4] |= 2u << (2 * (tail & 15));
      }
    }
    g4[2 * (size_t)idx] = mask;
    g4[2 * (size_t)idx + 1] = st;
    G.entry[3 * (size_t)(st - fv.depth_start[4])] = mask;
    G.entry[3 * (size_t)(st - fv.depth_start[4]) + 1] = fv.row_ptr[st + 1] > fv.row_ptr[st] ? fv.edge_next[fv.row_ptr[st]] : 0u;
    G.entry[3 * (size_t)(st - fv.depth_start[4]) + 2] = fv.term_kw[st] == NONE ? NONE : fv.term_kw[st] + G.kw_base;
    if (G.bloom) {
      auto set = [&] (uint32_t slot) { G.bloom[slot >> 5] |= 1u << (slot & 31); };
      if (fv.term_kw[st] != NONE) {
        set (gram_bloom_slot (gram_bloom_hash (idx, 0), G.bloomT_bits, 0));
        set (gram_bloom_slot (gram_bloom_hash (idx, 0), G.bloomT_bits, 1));
      }
      for (uint32_t e = fv.row_ptr[st]; e < fv.row_ptr[st + 1]; e++) {
        const uint32_t c5 = fv.edge_sym[e] - G.lo;
        set (G.bloomT_bits + gram_bloom_slot (gram_bloom_hash5 (idx, c5, 0), G.bloom5_bits, 0));
        set (G.bloomT_bits + gram_bloom_slot (gram_bloom_hash5 (idx, c5, 0), G.bloom5_bits, 1));
      }
    }
  }
  if (!G.wide) {
    const uint32_t words = (G.W * G.W * G.W * G.W + 31) / 32;
    uint32_t acc = 0;
    for (uint32_t w = 0; w < words; w++) {
      G.prefix[w] = acc;
      acc += (uint32_t)__builtin_popcount (bits[w]);
    }
  }
  if (G.shorts && G.wide) {
    uint32_t *stab = G.stab;
    for (uint32_t st = 1; st < fv.depth_start[4]; st++) {
      if (fv.term_kw[st] == NONE)
        continue;
      const uint32_t key = path[st] | (fv.depth[st] << 24);
      const uint32_t hb = (key * WIDE_H1) >> (32 - G.bloom_log2);
      bits[hb >> 5] |= 1u << (hb & 31);
      uint32_t slot = (key * WIDE_H2) >> (32 - G.stab_log2);
      while (stab[2 * (size_t)slot + 1])
        slot = (slot + 1) & ((1u << G.stab_log2) - 1);
      stab[2 * (size_t)slot] = key;
      stab[2 * (size_t)slot + 1] = G.kw_inline ? (fv.term_kw[st] + G.kw_base) | (fv.depth[st] << 28) | HIT_KW : st;
    }
  }
  if (G.shorts && !G.wide) {
    /* a keyword of d < 4 symbols with path p covers the 3-gram indices [p * W^(3-d), (p+1) * W^(3-d)) */
    unsigned char *nib = G.nib;
    uint32_t *g3 = G.g3;
    for (uint32_t st = 1; st < fv.depth_start[4]; st++) {
      if (fv.term_kw[st] == NONE)
        continue;
      const uint32_t d = fv.depth[st];
      uint32_t width = 1;
      for (uint32_t k = d; k < 3; k++)
        width *= G.W;
      for (uint32_t i3 = path[st] * width; i3 < (path[st] + 1) * width; i3++) {
        nib[i3 >> 1] |= (unsigned char)((1u << (d - 1)) << ((i3 & 1) * 4));
        g3[4 * (size_t)i3 + (d - 1)] = fv.term_kw[st] + G.kw_base; /* the keyword's id: its record is written on the spot */
      }
    }
  }
}

/* ---- plan construction (acm_gpu_plan_create_flat, and the delta plans of acm_gpu_plan_update).
 * One device allocation holds every table of a plan; its host image is built table by table: the
 * CSR tables every plan has, then those of the kernel family the dictionary qualifies for. */

/* the environment switches that shape a plan (experiments and tests), read once per plan */
struct PlanSwitches {
  int segment_log2 = env_int ("ACM_GPU_SEGMENT_LOG2", 0); /* launch segments of 2^12 .. 2^31 symbols */
  int gram = env_int ("ACM_GPU_GRAM", 1); /* 0: never the 4-gram kernel; 2: whenever the dictionary qualifies; 3: hashed windows always */
  bool bloom = env_int ("ACM_GPU_BLOOM", 1) != 0;          /* 0: no Bloom filters */
  bool gram2 = env_int ("ACM_GPU_GRAM2", 1) != 0;          /* 0: scan_gram_kernel instead of scan_gram2_kernel */
  bool peek8 = env_int ("ACM_GPU_PEEK8", 0) == 1;          /* 1: 8-byte peek entries whatever the size */
  bool sparse_walk = getenv ("ACM_GPU_SPARSE") && strcmp (getenv ("ACM_GPU_SPARSE"), "walk") == 0; /* the sparse walk, not the start-parallel kernel */
  bool short_blocks1 = env_int ("ACM_GPU_SHORT_BLOCKS", 0) == 1; /* 1: scan_short_kernel counts with one block a CU */
  int grid_blocks = env_int ("ACM_GPU_GRID_BLOCKS", 0);    /* fewer workgroups than CUs */
};

/* asked once per device: the call takes a good part of a millisecond, and the delta plans of
 * acm_gpu_plan_update are made at every dictionary change */
int
device_properties (int device, hipDeviceProp_t *prop) {
  int ndev = 0;
  if (hipGetDeviceCount (&ndev) != hipSuccess || ndev <= 0)
    return ACM_GPU_E_NODEVICE;
  if (device < 0 || device >= ndev)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (device));
  static std::mutex prop_mutex;
  static std::vector<std::pair<int, hipDeviceProp_t>> prop_cache;
  std::lock_guard<std::mutex> g (prop_mutex);
  for (const auto &c : prop_cache)
    if (c.first == device) {
      *prop = c.second;
      return ACM_GPU_OK;
    }
  HIP_TRY (hipGetDeviceProperties (prop, device));
  prop_cache.emplace_back (device, *prop);
  return ACM_GPU_OK;
}

/* a plan in the making: the flat tables, the switches, and the host image of the plan's device
 * allocation, grown table by table (256-byte aligned offsets) */
struct PlanBuild {
  const ACMFlat *flat;
  ACMFlatInfo fi;
  ACMFlatView fv;
  PlanSwitches sw;
  uint32_t lds_cap; /* dynamic LDS a workgroup can have: 160 KiB on gfx950 */
  uint32_t kw_base;
  std::vector<unsigned char> host;

  size_t
  reserve (size_t bytes) {
    size_t cur = host.size ();
    const size_t at = blob_reserve (cur, bytes);
    host.resize (cur, 0);
    return at;
  }
  template <typename T>
  T *
  at (size_t off) {
    return reinterpret_cast<T *> (host.data () + off);
  }
};

/* CSR tables (every plan: the CSR kernel takes any text), output info, depth_start */
struct CommonTables {
  size_t o_row, o_sym, o_next, o_fail, o_cnbo, o_oinfo, o_dstart;
};

void
build_common (PlanBuild &B, CommonTables &T) {
  const ACMFlatInfo &fi = B.fi;
  const ACMFlatView &fv = B.fv;
  const uint32_t n = fi.n_states;
  T.o_row = B.reserve (((size_t)n + 1) * 4);
  T.o_sym = B.reserve ((size_t)(fi.n_edges ? fi.n_edges : 1) * 4);
  T.o_next = B.reserve ((size_t)(fi.n_edges ? fi.n_edges : 1) * 4);
  T.o_fail = B.reserve ((size_t)n * 4);
  T.o_cnbo = B.reserve ((size_t)n * 4);
  T.o_oinfo = B.reserve ((size_t)n * 16);
  T.o_dstart = B.reserve (((size_t)fi.lmax + 2) * 4);
  memcpy (B.at<uint32_t> (T.o_row), fv.row_ptr, ((size_t)n + 1) * 4);
  memcpy (B.at<uint32_t> (T.o_sym), fv.edge_sym, (size_t)fi.n_edges * 4);
  memcpy (B.at<uint32_t> (T.o_next), fv.edge_next, (size_t)fi.n_edges * 4);
  memcpy (B.at<uint32_t> (T.o_fail), fv.fail, (size_t)n * 4);
  memcpy (B.at<uint32_t> (T.o_cnbo), fv.nb_outputs, (size_t)n * 4);
  uint32_t *oi = B.at<uint32_t> (T.o_oinfo);
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t nb = fv.nb_outputs[s];
    const uint32_t t0 = fv.term_kw[s] != NONE ? s : fv.out_link[s];
    oi[4 * s + 0] = nb;
    oi[4 * s + 1] = nb ? fv.out_link[t0] : 0;
    oi[4 * s + 2] = nb ? fv.depth[t0] : 0;
    oi[4 * s + 3] = nb ? fv.term_kw[t0] + B.kw_base : 0;
  }
  memcpy (B.at<uint32_t> (T.o_dstart), fv.depth_start, ((size_t)fi.lmax + 2) * 4);
}

void
bind_common (ACMPlan *p, const PlanBuild &B, const CommonTables &T, unsigned char *b) {
  auto u32p = [&] (size_t off) { return reinterpret_cast<const uint32_t *> (b + off); };
  p->csr.row_ptr = u32p (T.o_row);
  p->csr.edge_sym = u32p (T.o_sym);
  p->csr.edge_next = u32p (T.o_next);
  p->csr.fail = u32p (T.o_fail);
  p->csr.nb_outputs = u32p (T.o_cnbo);
  p->csr.lmax = B.fi.lmax;
  p->d_oinfo = reinterpret_cast<const uint4 *> (b + T.o_oinfo);
  p->d_dstart = u32p (T.o_dstart);
}

/* dense kernel (dev_dense.h), continuation or sticky mode: failure-resolved rows of every state;
 * LDS holds the rows of a breadth-first prefix [0, HD), continuation mode also hotfail (s) (2 bytes)
 * of every other state */
struct DenseTables {
  bool on = false, cont = false; /* cont: continuation mode (2-byte entries), see scan_dense_kernel */
  uint32_t entry_bytes = 0, rowbytes = 0, queue_bytes = 0, HD = 0, rows_lds = 0, hf_bytes = 0, image_bytes = 0;
  uint32_t lds_bytes = 0, lds_launch = 0; /* LDS in use; LDS a launch asks for (ACMPlan::dense_lds_launch) */
  std::vector<uint16_t> hotfail;
  size_t o_dense = 0, o_contdh = 0, o_wrows = 0, o_chain = 0, o_image = 0;
};

/* Chain records (EmitCtx::chain).  A continuation item says: walk on from rowless state s and
 * report what is longer than j + depth (hotfail (s)) after j more symbols.  When f(s) has a
 * row (hotfail (s) = f(s)), every failure transition out of the trie below s lands no deeper
 * than that bound, so the walk can only ever report along the goto path; and when that path
 * is a single chain of r <= 8 symbols to a leaf t with no keyword ending on the way, the
 * whole walk is one comparison of the next r text bytes: 2 independent loads instead of 4-8
 * dependent ones in expand_items_once_kernel. */
void
fill_chain_records (const ACMFlatView &fv, uint32_t n, const DenseTables &D, uint32_t *ch) {
  for (uint32_t s0 = D.HD; s0 < n; s0++) {
    uint32_t *r = ch + 4 * (size_t)(s0 - D.HD);
    const uint32_t dh = fv.depth[D.hotfail[s0]];
    if (fv.fail[s0] >= D.HD || dh >= 4000)
      continue;
    uint64_t syms = 0;
    uint32_t len = 0, st = s0;
    bool ok = true;
    while (fv.row_ptr[st + 1] > fv.row_ptr[st]) { /* until a leaf */
      if (fv.row_ptr[st + 1] - fv.row_ptr[st] != 1 || len == 8 || (st != s0 && fv.term_kw[st] != NONE)) {
        ok = false;
        break;
      }
      syms |= (uint64_t)(fv.edge_sym[fv.row_ptr[st]] & 0xFFu) << (8 * len);
      st = fv.edge_next[fv.row_ptr[st]];
      len++;
    }
    if (!ok)
      continue;
    r[0] = (len ? len : 15u) | (dh << 4);
    r[1] = st;
    r[2] = (uint32_t)syms;
    r[3] = (uint32_t)(syms >> 32);
  }
}

int
build_dense (PlanBuild &B, DenseTables &D) {
  const ACMFlatInfo &fi = B.fi;
  const ACMFlatView &fv = B.fv;
  const uint32_t n = fi.n_states;
  /* failure-resolved rows for byte alphabets whenever the whole DFA fits comfortably in HBM */
  D.entry_bytes = n <= 32768 ? 2 : 4;
  /* (the kernel's LDS layout is fixed at compile time for the 160 KiB of gfx950: DENSE_HF_END) */
  D.on = fi.sym_bytes == 1 && fi.n_edges > 0 && (uint64_t)n * fi.width < (1ull << 31) &&
         (uint64_t)n * fi.width * D.entry_bytes <= (8ull << 30) && fi.lmax >= 1 && fi.lmax - 1 <= 16u * 255 &&
         B.lds_cap == DENSE_LDS_CAP;
  D.cont = D.on && D.entry_bytes == 2;
  D.rowbytes = fi.width * D.entry_bytes;
  /* (-DACM_DENSE_DIRECT_PARK: the dense kernel parks its items straight into HBM, no LDS queues) */
  D.queue_bytes = DENSE_LDS_QUEUE ? (DENSE_THREADS / WAVE) * QCAP * 8 : 0;
  if (D.on) {
    const uint32_t budget = B.lds_cap - D.queue_bytes - 512;
    if (D.cont) {
      /* HD * rowbytes + (n - HD) * 2 <= budget */
      const uint64_t fixed = (uint64_t)n * 2;
      D.HD = fixed >= budget ? 1 : (uint32_t)((budget - fixed) / (D.rowbytes - 2));
    } else
      D.HD = budget / D.rowbytes;
    if (D.HD > n)
      D.HD = n;
    if (D.HD < 1)
      D.HD = 1;
  }
  if (D.cont) {
    D.hotfail.resize (n);
    for (uint32_t s = 0; s < n; s++) /* f(s) < s: one pass in breadth-first order */
      D.hotfail[s] = (uint16_t)(s < D.HD ? s : D.hotfail[fv.fail[s]]);
  }
  /* (the rows and the LDS image take 16 bytes of the blob in plans without rows too) */
  D.o_dense = B.reserve ((D.on ? (size_t)n * D.rowbytes : 0) + 16);
  D.o_contdh = B.reserve (D.cont ? (size_t)n * 2 : 0);
  D.o_wrows = B.reserve (D.cont ? (size_t)n * fi.width * 4 : 0);
  D.o_chain = B.reserve (D.cont ? (size_t)(n - D.HD) * 16 + 16 : 0);
  /* LDS: [HD rows][16 queues][tile counter] from address 0 and, continuation mode with rowless
   * states, their hotfail in descending order below DENSE_HF_END (dev_all.h); the image holds the
   * two parts back to back, each a multiple of 16 bytes */
  D.rows_lds = D.on ? ((D.HD * D.rowbytes + 15) & ~15u) : 0;
  D.hf_bytes = D.cont ? (((n - D.HD) * 2 + 15) & ~15u) : 0;
  D.image_bytes = D.rows_lds + D.hf_bytes;
  D.lds_bytes = D.image_bytes + D.queue_bytes + 16 /* tile counter */;
  /* (continuation mode always up to DENSE_HF_END: its slow step reads there in every lane) */
  D.lds_launch = D.cont ? DENSE_HF_END : D.lds_bytes;
  D.o_image = B.reserve (D.image_bytes + 16);
  if (!D.on)
    return ACM_GPU_OK;
  if (D.rows_lds + D.queue_bytes + 16 + D.hf_bytes > DENSE_HF_END) /* (the budget above rules it out) */
    return ACM_GPU_E_INELIGIBLE;
  int rc = acm_flat_dense_rows (B.flat, n, D.entry_bytes, B.at<unsigned char> (D.o_dense));
  if (rc)
    return rc;
  /* LDS image: the first HD rows, then hotfail of the states n - 1, n - 2, ..., HD */
  memcpy (B.at<unsigned char> (D.o_image), B.at<unsigned char> (D.o_dense), (size_t)D.HD * D.rowbytes);
  if (D.cont) {
    const uint16_t *r16 = B.at<uint16_t> (D.o_dense);
    uint32_t *wr = B.at<uint32_t> (D.o_wrows);
    for (size_t i = 0; i < (size_t)n * fi.width; i++)
      wr[i] = r16[i] | (fv.depth[r16[i] & 0x7FFFu] << 16);
    uint16_t *cdh = B.at<uint16_t> (D.o_contdh);
    for (uint32_t s = 0; s < n; s++)
      cdh[s] = (uint16_t)fv.depth[D.hotfail[s]];
    uint16_t *hf = B.at<uint16_t> (D.o_image + D.rows_lds);
    const uint32_t hf_slots = D.hf_bytes / 2;
    for (uint32_t i = 0; i < hf_slots; i++) /* slot hf_slots - 1 is state HD; the slots of the rounding come first */
      hf[i] = hf_slots - 1 - i < n - D.HD ? D.hotfail[D.HD + (hf_slots - 1 - i)] : 0;
    fill_chain_records (fv, n, D, B.at<uint32_t> (D.o_chain));
  }
  return ACM_GPU_OK;
}

void
bind_dense (ACMPlan *p, const PlanBuild &B, const DenseTables &D, unsigned char *b) {
  const ACMFlatInfo &fi = B.fi;
  p->entry_bytes = D.entry_bytes;
  if (!D.on)
    return;
  p->kind = PlanKind::Dense;
  p->d_dense = b + D.o_dense;
  p->d_lds_image = b + D.o_image;
  p->d_cont_dh = D.cont ? reinterpret_cast<const uint16_t *> (b + D.o_contdh) : nullptr;
  p->d_chain = D.cont ? reinterpret_cast<const uint4 *> (b + D.o_chain) : nullptr;
  p->d_wrows = D.cont ? reinterpret_cast<const uint32_t *> (b + D.o_wrows) : nullptr;
  p->lds_image_bytes = D.image_bytes;
  p->dense_lds_launch = D.lds_launch;
  DenseK &K = p->K;
  K.W = fi.width;
  K.rowbytes = D.rowbytes;
  K.lo = fi.alpha_lo;
  K.span = fi.alpha_span;
  K.HD = D.HD;
  K.rows_bytes = D.rows_lds;
  K.queue_off = D.rows_lds;
  K.wub = fi.lmax > 1 ? (fi.lmax - 1 + 15) / 16 : 0;
  K.lmax = fi.lmax;
  K.stream_stride = WAVE * p->chunk;
}

/* 4-gram sieve kernel (dev_gram.h, dev_gram2.h, dev_short.h): sizes and places of its tables */
struct GramTables {
  bool on = false;     /* the tables are made (the plan takes the kernel if they fit LDS: bind_gram) */
  bool hashed = false; /* wide alphabets: hashed 4-byte windows instead of the exact base-W index */
  bool shorts = false; /* keywords of 1-3 symbols */
  bool gram2 = false;
  uint32_t n_depth4 = 0, bits_bytes = 0, tab2_words = 0, g2_off = 0;
  GramK K{}; /* the kernel's sizes (bind_gram adds the pointers) */
  size_t o_g4bits, o_g3rec, o_stab, o_shimg, o_g4rec, o_grec, o_gedge, o_g4gid, o_kw4, o_g4prefix, o_g4entry, o_g5peek, o_tab2, o_rows2, o_over2;
};

/* LDS of the waves' queues (hit queue, walk queues, short-keyword queue of hashed windows) */
uint32_t
gram_queue_bytes (const GramTables &G) {
  return (SPARSE_THREADS / WAVE) * ((G.shorts && G.hashed ? QCAP : 0u) + GRAM_Q1 + GRAM_Q2 + (G.hashed ? HITS_STRIDE : 0u)) * 8;
}

/* narrow alphabets: what LDS has left after the bits and the queues goes to the two Bloom filters
 * of the record gather (GramK::bloom5_bits): 8 to 16 bits per terminal 4-gram, the rest for the
 * 5-grams; not worth it below 4 bits per 5-gram or for dictionaries of a few hundred keywords */
void
size_gram_bloom (const PlanBuild &B, GramTables &G) {
  const ACMFlatView &fv = B.fv;
  GramK &K = G.K;
  if (!G.on || G.hashed || G.n_depth4 < 2048 || !B.sw.bloom)
    return;
  K.bloom_off = (K.g3_off + K.g3_bytes + 15) & ~15u;
  const uint64_t used = (uint64_t)K.bloom_off + gram_queue_bytes (G) + WALK_CTX_BYTES + 64;
  uint32_t n_term4 = 0, n_5 = 0;
  for (uint32_t st = fv.depth_start[4]; st < fv.depth_start[5]; st++) {
    n_term4 += fv.term_kw[st] != NONE ? 1u : 0u;
    n_5 += fv.row_ptr[st + 1] - fv.row_ptr[st];
  }
  if (used >= B.lds_cap)
    return;
  const uint64_t free_bits = ((uint64_t)B.lds_cap - used) / 16 * 16 * 8;
  uint64_t tb = (uint64_t)n_term4 * 12 + 1024;
  if (tb > free_bits / 3)
    tb = free_bits / 3;
  tb = tb / 128 * 128;
  const uint64_t fb = (free_bits - tb) / 128 * 128;
  if (tb >= 1024 && fb >= (uint64_t)n_5 * 2 && fb < (1u << 24)) {
    K.bloomT_bits = (uint32_t)tb;
    K.bloom5_bits = (uint32_t)fb;
  }
}

/* Which byte dictionaries get the 4-gram tables, and their sizes and places in the blob.  They are
 * the dictionaries that the LDS scheme of the dense kernel does not serve well: every automaton of
 * more than 32,768 states, and the smaller ones whose hot set outgrows LDS: the share of a uniform
 * text's positions that land in a state without an LDS row is estimated as the sum over those
 * states of span^-depth; above 0.1 % the continuation items swamp the dense kernel (measured on
 * a-z, ms per GiB, dense against 4-gram: 1,100 keywords 0.06 % -> 0.38 / 0.41; 1,250 keywords
 * 0.13 % -> 0.46 / 0.42; 1,500 keywords 0.26 % -> 0.58 / 0.43; 3,000 keywords -> 9.0 / 0.48). */
int
build_gram (PlanBuild &B, const DenseTables &D, GramTables &G) {
  const ACMFlatInfo &fi = B.fi;
  const ACMFlatView &fv = B.fv;
  const uint32_t n = fi.n_states;
  GramK &K = G.K;
  double rowless_share = 0;
  if (D.cont && fi.alpha_span > 1) {
    for (uint32_t s = D.HD; s < n; s++)
      rowless_share += pow ((double)fi.alpha_span, -(double)fv.depth[s]);
  }
  const bool narrow = fi.width <= 30 && fi.width == fi.alpha_span + 1 && B.sw.gram != 3;
  bool any_short = false;
  for (uint32_t k = 0; k < fi.n_keywords; k++)
    any_short |= fv.depth[fv.kw_state[k]] < 4;
  G.on = D.on && (D.entry_bytes == 4 || B.sw.gram >= 2 || rowless_share > 0.001) && B.sw.gram != 0 && fi.lmax >= 4 && n < 0x40000000u;
  if (!G.on) {
    B.reserve (0); /* (the blob ends on a 256-byte boundary, as it always did behind the 4-gram tables) */
    return ACM_GPU_OK;
  }
  G.shorts = any_short; /* a nibble per 3-gram + their ids (narrow: a pass of their own, scan_short_kernel; hashed: the kernel's third queue) */
  G.hashed = !narrow;
  const bool hashed = G.hashed, narrow_shorts = G.shorts && !hashed;
  const uint32_t gW = K.W = fi.width;
  K.lo = fi.alpha_lo;
  K.span = fi.alpha_span;
  K.bloom_log2 = 19; /* hashed: 64 KB of Bloom bits */
  G.n_depth4 = fv.depth_start[5] - fv.depth_start[4];
  K.wtab_log2 = 4;
  while (hashed && (1u << K.wtab_log2) < 2 * G.n_depth4 + 2)
    K.wtab_log2++;
  uint32_t n_short = 0; /* hashed windows: keywords of 1-3 symbols */
  for (uint32_t k = 0; k < fi.n_keywords && hashed && G.shorts; k++)
    if (fv.depth[fv.kw_state[k]] < 4) {
      n_short++;
      K.short_lens |= 1u << (fv.depth[fv.kw_state[k]] - 1);
    }
  K.stab_log2 = 4;
  while ((1u << K.stab_log2) < 2 * n_short + 2)
    K.stab_log2++;
  K.W4 = hashed ? 1u << K.wtab_log2 : gW * gW * gW * gW; /* 8-byte records of the second stage */
  K.g4words = hashed ? (1u << K.bloom_log2) / 32 : (K.W4 + 31) / 32;
  const uint32_t W3 = !hashed ? gW * gW * gW : 0;
  K.g3_off = (K.g4words * 4 + 15) & ~15u; /* nibble table right after the 4-gram bits */
  K.g3_bytes = narrow_shorts ? ((W3 + 1) / 2 + 15) & ~15u : 0;
  size_gram_bloom (B, G);
  G.bits_bytes = K.bloom5_bits ? K.bloom_off + (K.bloomT_bits + K.bloom5_bits) / 8 : K.g3_off + K.g3_bytes;
  /* scan_gram2_kernel (dev_gram2.h: lane-local sieve on two bits per 4-gram, no queue push per
   * position, no Bloom filters): narrow alphabets whose table fits LDS beside the waves' areas --
   * up to 26 symbols + "other".  ACM_GPU_GRAM2=0: scan_gram_kernel. */
  G.tab2_words = !hashed ? (K.W4 + 15) / 16 : 0;
  G.g2_off = (G.tab2_words * 4 + 15) & ~15u;
  G.gram2 = !hashed && B.sw.gram2 && (uint64_t)G.g2_off + G2_LDS_FIXED <= B.lds_cap;
  G.o_g4bits = B.reserve ((size_t)G.bits_bytes + 16);
  G.o_g3rec = B.reserve (narrow_shorts ? (size_t)W3 * 16 : 0);
  G.o_stab = B.reserve (hashed && G.shorts ? ((size_t)8 << K.stab_log2) : 0);
  /* scan_short_kernel's LDS image: the nibbles, the number of set nibble bits in front of every 8
   * 3-grams, the keyword ids in the order of those bits (a keyword of d symbols is the id of W^(3-d) 3-grams) */
  uint32_t sh_ids = 0;
  for (uint32_t st = 1; narrow_shorts && st < fv.depth_start[4]; st++)
    if (fv.term_kw[st] != NONE)
      sh_ids += fv.depth[st] == 1 ? gW * gW : (fv.depth[st] == 2 ? gW : 1u);
  K.sh_nib_bytes = K.g3_bytes;
  K.sh_base_bytes = narrow_shorts ? (((W3 + 7) / 8) * 4 + 15) & ~15u : 0;
  K.sh_ids_bytes = (sh_ids * 4 + 15) & ~15u;
  G.o_shimg = B.reserve (narrow_shorts ? (size_t)K.sh_nib_bytes + K.sh_base_bytes + K.sh_ids_bytes + 16 : 0);
  G.o_g4rec = B.reserve ((size_t)K.W4 * 8);
  G.o_grec = B.reserve ((size_t)n * 32);
  G.o_gedge = B.reserve ((size_t)fi.n_edges * 8);
  K.d4_begin = fv.depth_start[4];
  K.d5_begin = fv.depth_start[5]; /* (lmax >= 4: depth_start has lmax + 2 entries) */
  G.o_g4gid = B.reserve ((size_t)(K.d5_begin - K.d4_begin) * 4 + 16);
  G.o_kw4 = B.reserve ((size_t)G.n_depth4 * 4 + 16);
  G.o_g4prefix = B.reserve (!hashed ? (size_t)K.g4words * 4 + 16 : 0);
  G.o_g4entry = B.reserve (!hashed ? (size_t)G.n_depth4 * 12 + 16 : 0);
  const uint32_t n_depth5 = fi.lmax >= 5 ? fv.depth_start[6] - fv.depth_start[5] : 0;
  /* peek entries of 4 bytes while a record index fits 23 bits (ACM_GPU_PEEK8=1: 8 bytes anyway -- tests) */
  K.peek_packed = n < (1u << 23) && !B.sw.peek8 ? 1u : 0u;
  K.d5_rel = K.peek_packed; /* (fewer than 2^23 states in all: a record index leaves bits 24-29 free too) */
  K.kw_inline = (uint64_t)fi.n_keywords + B.kw_base <= HIT_KW_ID ? 1u : 0u;
  K.queue_off = G.bits_bytes;
  G.o_g5peek = B.reserve (!hashed ? (size_t)n_depth5 * (K.peek_packed ? 4 : 8) + 16 : 0);
  G.o_tab2 = B.reserve (G.gram2 ? (size_t)G.g2_off + 16 : 0);
  /* (the second stage's entries by row, with scan_gram2_kernel: classes are below 30, bits 30 and 31 are flags) */
  G.o_rows2 = B.reserve (G.gram2 ? (size_t)G.tab2_words * 64 + 16 : 0);
  G.o_over2 = B.reserve (G.gram2 ? (size_t)G.n_depth4 * 8 + 16 : 0);

  /* the host image: fill_gram_tables, the keyword ids of the depth-4 states, scan_short_kernel's image */
  GramImage I{ hashed, G.shorts, gW, K.bloom_log2, K.wtab_log2, K.stab_log2 };
  I.bits = B.at<uint32_t> (G.o_g4bits);
  I.g4 = B.at<uint32_t> (G.o_g4rec);
  I.rec = B.at<uint32_t> (G.o_grec);
  I.edge = B.at<uint32_t> (G.o_gedge);
  I.g4gid = B.at<uint32_t> (G.o_g4gid);
  I.nib = B.at<unsigned char> (G.o_g4bits + K.g3_off);
  I.prefix = B.at<uint32_t> (G.o_g4prefix);
  I.entry = B.at<uint32_t> (G.o_g4entry);
  I.peek = hashed ? nullptr : B.at<uint32_t> (G.o_g5peek);
  I.bloom = K.bloom5_bits ? B.at<uint32_t> (G.o_g4bits + K.bloom_off) : nullptr;
  I.bloomT_bits = K.bloomT_bits;
  I.bloom5_bits = K.bloom5_bits;
  I.lo = fi.alpha_lo;
  I.kw_base = B.kw_base;
  I.kw_inline = K.kw_inline != 0;
  I.peek_packed = K.peek_packed != 0;
  I.g3 = B.at<uint32_t> (G.o_g3rec);
  I.stab = B.at<uint32_t> (G.o_stab);
  I.tab2 = G.gram2 ? B.at<uint32_t> (G.o_tab2) : nullptr;
  I.rows2 = G.gram2 ? B.at<uint32_t> (G.o_rows2) : nullptr;
  I.over2 = G.gram2 ? B.at<uint32_t> (G.o_over2) : nullptr;
  fill_gram_tables (fv, fi, I);
  for (uint32_t st = fv.depth_start[4]; st < fv.depth_start[5]; st++)
    B.at<uint32_t> (G.o_kw4)[st - fv.depth_start[4]] = fv.term_kw[st] == NONE ? NONE : fv.term_kw[st] + B.kw_base;
  if (!narrow_shorts)
    return ACM_GPU_OK;
  unsigned char *img = B.at<unsigned char> (G.o_shimg);
  memcpy (img, I.nib, (W3 + 1) / 2);
  uint32_t *base = reinterpret_cast<uint32_t *> (img + K.sh_nib_bytes), *ids = reinterpret_cast<uint32_t *> (img + K.sh_nib_bytes + K.sh_base_bytes);
  uint32_t r = 0;
  for (uint32_t i3 = 0; i3 < W3; i3++) {
    if ((i3 & 7) == 0)
      base[i3 >> 3] = r;
    const uint32_t nb = (I.nib[i3 >> 1] >> ((i3 & 1) * 4)) & 7u;
    for (uint32_t d = 0; d < 3; d++)
      if ((nb >> d) & 1u)
        ids[r++] = I.g3[4 * (size_t)i3 + d];
  }
  return r == sh_ids ? ACM_GPU_OK : ACM_GPU_E_ARG; /* (the two counts are of the same keywords) */
}

/* The plan takes the 4-gram kernel when its bits and queues fit LDS; else it stays a dense plan,
 * with the 4-gram tables left unused in its blob. */
void
bind_gram (ACMPlan *p, const PlanBuild &B, const GramTables &G, unsigned char *b) {
  if (!G.on || (uint64_t)G.bits_bytes + gram_queue_bytes (G) + WALK_CTX_BYTES > B.lds_cap)
    return;
  auto u32p = [&] (size_t off) { return reinterpret_cast<const uint32_t *> (b + off); };
  p->kind = PlanKind::Gram;
  p->hashed = G.hashed;
  p->inline_shorts = G.shorts && G.hashed;
  p->short_pass = G.shorts && !G.hashed;
  p->gram2 = G.gram2;
  p->d_kw4 = u32p (G.o_kw4);
  GramK &K = p->GK;
  K = G.K;
  K.g4prefix = u32p (G.o_g4prefix);
  K.g4entry = u32p (G.o_g4entry);
  K.g5peek = u32p (G.o_g5peek);
  K.g4rec = reinterpret_cast<const uint2 *> (b + G.o_g4rec);
  K.g4bits = u32p (G.o_g4bits);
  K.srec = reinterpret_cast<const uint4 *> (b + G.o_grec);
  K.sedge = reinterpret_cast<const uint2 *> (b + G.o_gedge);
  K.g4gid = u32p (G.o_g4gid);
  K.g3rec = reinterpret_cast<const uint4 *> (b + G.o_g3rec);
  K.wtab = reinterpret_cast<const uint2 *> (b + G.o_g4rec);
  K.stab = reinterpret_cast<const uint2 *> (b + G.o_stab);
  K.sh_img = u32p (G.o_shimg);
  /* the ids in LDS too while they fit (29 K of them beside the tables and the waves' areas) */
  p->short_ids_lds = (uint64_t)K.sh_nib_bytes + K.sh_base_bytes + K.sh_ids_bytes + SH_LDS_FIXED <= B.lds_cap;
  p->short_lds_bytes = K.sh_nib_bytes + K.sh_base_bytes + (p->short_ids_lds ? K.sh_ids_bytes : 0u) + SH_LDS_FIXED;
  p->short_lds_count_bytes = K.sh_nib_bytes + SH_LDS_FIXED;
  p->short_blocks_per_cu = 2u * (K.sh_nib_bytes + SH_LDS_FIXED) <= 160u * 1024u ? 2u : 1u; /* (count-only: the nibbles alone) */
  if (B.sw.short_blocks1)
    p->short_blocks_per_cu = 1;
  p->gram_lds_bytes = G.bits_bytes + gram_queue_bytes (G) + WALK_CTX_BYTES;
  if (G.gram2) {
    K.rows2 = reinterpret_cast<const uint2 *> (b + G.o_rows2);
    K.over2 = reinterpret_cast<const uint2 *> (b + G.o_over2);
    K.tab2 = u32p (G.o_tab2);
    K.tab2_words = G.tab2_words;
    K.g2_off = G.g2_off;
    p->gram_lds_bytes = G.g2_off + G2_LDS_FIXED;
  }
}

/* 2- and 4-byte symbols: the sparse walk's tables (state records, (symbol, next) edges, root table by
 * symbol value) and, for fewer than 2^30 states, the same three for the start-parallel kernel (flags
 * mean something else there) and its pair table.  A start-parallel plan keeps the sparse tables:
 * a segment of text that is not 16-byte aligned takes the sparse walk. */
struct SparseTables {
  bool on = false, starts = false;
  uint32_t lut_size = 0;
  size_t o_srec, o_sedge, o_lut, o_trec, o_tedge, o_tlut, o_tpairs;
};

void
build_sparse (PlanBuild &B, const DenseTables &D, SparseTables &S) {
  const ACMFlatInfo &fi = B.fi;
  const ACMFlatView &fv = B.fv;
  const uint32_t n = fi.n_states;
  S.on = !D.on && fi.sym_bytes >= 2 && fi.n_edges > 0 && n < 0x7FFFFFFFu;
  if (!S.on)
    return;
  const uint32_t root_edges = fv.row_ptr[1];
  const uint64_t top = root_edges ? (uint64_t)fv.edge_sym[root_edges - 1] + 1 : 0; /* rows are in ascending order */
  S.lut_size = (uint32_t)(top < (1ull << 22) ? top : (1ull << 22));
  S.lut_size = (S.lut_size + 3) & ~3u;
  S.starts = n < 0x40000000u;
  S.o_srec = B.reserve ((size_t)n * 32);
  S.o_sedge = B.reserve ((size_t)fi.n_edges * 8);
  S.o_lut = B.reserve ((size_t)S.lut_size * 4 + 16);
  if (S.starts) {
    S.o_trec = B.reserve ((size_t)n * 32);
    S.o_tedge = B.reserve ((size_t)fi.n_edges * 8);
    S.o_tlut = B.reserve ((size_t)S.lut_size * 4 + 16);
    S.o_tpairs = B.reserve ((size_t)n * 8); /* by state id; filled for the root's children */
  }
  fill_sparse_tables (fv, fi, S.lut_size, B.at<uint32_t> (S.o_srec), B.at<uint32_t> (S.o_sedge), B.at<uint32_t> (S.o_lut));
  if (S.starts)
    fill_starts_tables (fv, fi, S.lut_size, B.at<uint32_t> (S.o_trec), B.at<uint32_t> (S.o_tedge), B.at<uint32_t> (S.o_tlut),
                        B.at<uint32_t> (S.o_tpairs));
}

/* what acm_gpu_plan_update edits: the host copy of the start-parallel tables (nullptr when out of memory) */
StartsMirror *
make_starts_mirror (PlanBuild &B, const SparseTables &S, size_t o_oinfo, unsigned char *b) {
  const ACMFlatInfo &fi = B.fi;
  const ACMFlatView &fv = B.fv;
  const uint32_t n = fi.n_states;
  StartsMirror *M = new (std::nothrow) StartsMirror ();
  if (!M)
    return nullptr;
  auto words = [&] (size_t off, size_t cnt) {
    const uint32_t *w = B.at<uint32_t> (off);
    return std::vector<uint32_t> (w, w + cnt);
  };
  M->tab[PT_REC] = words (S.o_trec, (size_t)n * 8);
  M->tab[PT_EDGE] = words (S.o_tedge, (size_t)fi.n_edges * 2);
  M->tab[PT_LUT] = words (S.o_tlut, S.lut_size);
  M->tab[PT_PAIRS] = words (S.o_tpairs, (size_t)n * 2);
  M->tab[PT_OINFO] = words (o_oinfo, (size_t)n * 4);
  M->parent.assign (n, 0);
  M->parent_sym.assign (n, 0);
  M->depth.assign (fv.depth, fv.depth + n);
  for (uint32_t st = 0; st < n; st++) {
    M->tab[PT_REC][8 * (size_t)st] = st ? fv.row_ptr[st + 1] - fv.row_ptr[st] : M->tab[PT_REC][1]; /* row capacity = its size */
    for (uint32_t e = fv.row_ptr[st]; e < fv.row_ptr[st + 1]; e++) {
      M->parent[fv.edge_next[e]] = st;
      M->parent_sym[fv.edge_next[e]] = fv.edge_sym[e];
    }
  }
  M->dev[PT_REC] = reinterpret_cast<uint32_t *> (b + S.o_trec);
  M->dev[PT_EDGE] = reinterpret_cast<uint32_t *> (b + S.o_tedge);
  M->dev[PT_LUT] = reinterpret_cast<uint32_t *> (b + S.o_tlut);
  M->dev[PT_PAIRS] = reinterpret_cast<uint32_t *> (b + S.o_tpairs);
  M->dev[PT_OINFO] = reinterpret_cast<uint32_t *> (b + o_oinfo);
  M->cap[PT_LUT] = S.lut_size;
  M->n_states = n;
  M->n_edges = fi.n_edges;
  M->n_keywords = fi.n_keywords;
  M->lmax = fi.lmax;
  return M;
}

void
bind_sparse (ACMPlan *p, PlanBuild &B, const SparseTables &S, size_t o_oinfo, unsigned char *b) {
  const ACMFlatInfo &fi = B.fi;
  if (!S.on)
    return;
  const uint32_t tps = 128 / fi.sym_bytes;
  const uint32_t warm = fi.lmax > 1 ? fi.lmax - 1 : 0;
  const uint32_t sparse_queue_bytes = (SPARSE_THREADS / WAVE) * QCAP * 8;
  p->kind = S.starts && !B.sw.sparse_walk ? PlanKind::Starts : PlanKind::Sparse;
  p->sparse_lut_lds = (uint64_t)S.lut_size * 4 + sparse_queue_bytes + 512 <= B.lds_cap;
  p->SK.srec = reinterpret_cast<const uint4 *> (b + S.o_srec);
  p->SK.sedge = reinterpret_cast<const uint2 *> (b + S.o_sedge);
  p->SK.lut = reinterpret_cast<const uint32_t *> (b + S.o_lut);
  p->SK.lut_size = S.lut_size;
  p->SK.warm_subs = (warm + tps - 1) / tps;
  p->SK.warm_skip = p->SK.warm_subs * tps - warm;
  p->SK.queue_off = p->sparse_lut_lds ? S.lut_size * 4 : 0;
  p->SK.R = 0; /* per launch */
  p->sparse_lds_bytes = p->SK.queue_off + sparse_queue_bytes + 16;
  if (!S.starts)
    return;
  p->TK.srec = reinterpret_cast<const uint4 *> (b + S.o_trec);
  p->TK.sedge = reinterpret_cast<const uint2 *> (b + S.o_tedge);
  p->TK.lut = reinterpret_cast<const uint32_t *> (b + S.o_tlut);
  p->TK.pairs = reinterpret_cast<const uint2 *> (b + S.o_tpairs);
  p->TK.lut_size = S.lut_size;
  const uint32_t starts_queue_bytes = (SPARSE_THREADS / WAVE) * (QCAP + HITS_STRIDE) * 8;
  p->starts_lut_lds = (uint64_t)S.lut_size * 4 + starts_queue_bytes + WALK_CTX_BYTES <= B.lds_cap;
  p->TK.queue_off = p->starts_lut_lds ? S.lut_size * 4 : 0;
  p->TK.R = 0;
  p->starts_lds_bytes = p->TK.queue_off + starts_queue_bytes + WALK_CTX_BYTES;
  if (p->kind == PlanKind::Starts)
    p->mir = make_starts_mirror (B, S, o_oinfo, b);
}

/* ACMPlanInfo of a plan whose tables are made and bound */
void
fill_plan_info (ACMPlan *p, const DenseTables &D) {
  ACMPlanInfo &I = p->info;
  I.device = p->device;
  I.kernel = (uint32_t)p->kind;
  I.entry_bytes = D.on ? D.entry_bytes : 0;
  I.width = p->finfo.width;
  I.dense_rows = D.on ? p->finfo.n_states : 0;
  I.lds_rows = D.HD;
  I.lds_hotfail = D.cont ? p->finfo.n_states - D.HD : 0;
  I.table_bytes = p->blob_bytes;
  I.chunk_bytes = p->chunk;
  I.streams = p->streams;
  I.grid_blocks = (uint32_t)p->cu_count;
  I.block_threads = SPARSE_THREADS;
  switch (p->kind) {
  case PlanKind::Dense:
    I.lds_bytes = D.lds_bytes;
    I.block_threads = DENSE_THREADS;
    break;
  case PlanKind::Csr:
    I.lds_bytes = QCAP * 8;
    I.block_threads = WAVE;
    I.grid_blocks = (uint32_t)p->cu_count * 16;
    break;
  case PlanKind::Sparse:
  case PlanKind::Starts:
    I.lds_bytes = p->kind == PlanKind::Starts ? p->starts_lds_bytes : p->sparse_lds_bytes;
    I.streams = p->kind == PlanKind::Starts ? 1 : SPARSE_S;
    I.chunk_bytes = 128;
    break;
  case PlanKind::Gram:
    I.lds_bytes = p->gram_lds_bytes;
    I.streams = 1;
    I.chunk_bytes = 16;
    break;
  }
}

/* every table of the plan: host image, one device allocation, pointers */
int
build_tables (PlanBuild &B, ACMPlan *p) {
  CommonTables T;
  DenseTables D;
  SparseTables S;
  GramTables G;
  build_common (B, T);
  int rc = build_dense (B, D);
  if (rc)
    return rc;
  build_sparse (B, D, S);
  rc = build_gram (B, D, G); /* (last: the blob's size, table_bytes, is what it always was) */
  if (rc)
    return rc;
  const size_t bytes = B.host.size ();
  p->blob_bytes = bytes;
  if (hipMalloc (&p->blob, bytes) != hipSuccess)
    return ACM_GPU_E_NOMEM;
  if (hipMemcpy (p->blob, B.host.data (), bytes, hipMemcpyHostToDevice) != hipSuccess)
    return ACM_GPU_E_HIP;
  const size_t ctl_bytes = 16 + 2 * POOL_CLASSES * POOL_CTR_STRIDE * sizeof (unsigned int);
  if (hipMalloc (reinterpret_cast<void **> (&p->scratch.d_total), ctl_bytes) != hipSuccess || hipMemset (p->scratch.d_total, 0, ctl_bytes) != hipSuccess)
    return ACM_GPU_E_NOMEM;
  p->scratch.d_pool_ctr = reinterpret_cast<unsigned int *> (p->scratch.d_total + 2);
  unsigned char *b = static_cast<unsigned char *> (p->blob);
  bind_common (p, B, T, b);
  bind_dense (p, B, D, b);
  bind_gram (p, B, G, b);
  bind_sparse (p, B, S, T.o_oinfo, b);
  fill_plan_info (p, D);
  return ACM_GPU_OK;
}

/* the dynamic LDS of the kernels the plan launches */
int
set_lds_attributes (const ACMPlan *p) {
  for (int co = 0; co < 2; co++) {
    switch (p->kind) {
    case PlanKind::Dense:
      HIP_TRY (hipFuncSetAttribute (dense_kernel (p, co != 0), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)p->dense_lds_launch));
      break;
    case PlanKind::Starts:
      HIP_TRY (hipFuncSetAttribute (starts_kernel (p, co != 0), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)p->starts_lds_bytes));
      [[fallthrough]]; /* (the sparse walk takes the segments that are not 16-byte aligned) */
    case PlanKind::Sparse:
      HIP_TRY (hipFuncSetAttribute (sparse_kernel (p, co != 0), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)p->sparse_lds_bytes));
      break;
    case PlanKind::Gram:
      HIP_TRY (hipFuncSetAttribute (gram_kernel (p, co != 0, false), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)p->gram_lds_bytes));
      if (p->short_pass)
        HIP_TRY (hipFuncSetAttribute (short_kernel (p, co != 0), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(co ? p->short_lds_count_bytes : p->short_lds_bytes)));
      break;
    case PlanKind::Csr: break;
    }
  }
  if (p->kind == PlanKind::Gram && !p->hashed)
    HIP_TRY (hipFuncSetAttribute (gram_kernel (p, false, true), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)p->gram_lds_bytes));
  return ACM_GPU_OK;
}

/* 8-byte symbols: hash table {key, id} of the dictionary's symbols, through which the text is interned */
int
upload_intern_table (ACMPlan *p, const ACMFlatView &fv) {
  uint32_t cap = 16;
  while (cap < 2 * (fv.n_keys64 + 1))
    cap <<= 1;
  std::vector<uint32_t> tab ((size_t)cap * 4, 0);
  auto mix = [] (uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
  };
  for (uint32_t k = 0; k < fv.n_keys64; k++) {
    const uint64_t key = fv.keys64[k];
    uint32_t h = (uint32_t)mix (key) & (cap - 1);
    while (tab[4 * (size_t)h + 2])
      h = (h + 1) & (cap - 1);
    tab[4 * (size_t)h] = (uint32_t)key;
    tab[4 * (size_t)h + 1] = (uint32_t)(key >> 32);
    tab[4 * (size_t)h + 2] = k + 1;
  }
  if (hipMalloc (reinterpret_cast<void **> (&p->d_intern), (size_t)cap * 16) != hipSuccess ||
      hipMemcpy (p->d_intern, tab.data (), (size_t)cap * 16, hipMemcpyHostToDevice) != hipSuccess)
    return ACM_GPU_E_NOMEM;
  p->intern_mask = cap - 1;
  return ACM_GPU_OK;
}

/* what maps a text to the symbols the kernels walk: the intern table of 8-byte symbols, the
 * comparator classes of 4-byte symbols (cls32), the class LUT of 1- and 2-byte symbols */
int
build_text_side (ACMPlan *p, const PlanBuild &B, bool interned) {
  const ACMFlatView &fv = B.fv;
  if (interned) {
    int rc = upload_intern_table (p, fv);
    if (rc)
      return rc;
  }
  if (fv.keys32 || (B.fi.sym_bytes == 4 && fv.class_rep32)) {
    p->cls32 = true;
    for (uint32_t i = 0; i < fv.n_keys32; i++)
      p->cls32_known[fv.keys32[i]] = fv.keys32_class[i];
    p->cls32_reps.assign (fv.class_rep32, fv.class_rep32 + fv.n_classes);
    if (hipMalloc (reinterpret_cast<void **> (&p->d_unknown), (size_t)(p->cls32_cap + 1) * 4) != hipSuccess)
      return ACM_GPU_E_NOMEM;
  }
  if (fv.class_map) {
    /* 65,536 entries either way: 2-byte symbols directly, bytes in pairs (see classmap_kernel) */
    std::vector<uint16_t> lut (65536);
    if (B.fi.sym_bytes == 1) {
      for (uint32_t v = 0; v < 65536; v++)
        lut[v] = (uint16_t)((fv.class_map[v >> 8] << 8) | (fv.class_map[v & 255] & 255));
    } else
      memcpy (lut.data (), fv.class_map, 65536 * 2);
    if (hipMalloc (reinterpret_cast<void **> (&p->d_classlut), 65536 * 2) != hipSuccess ||
        hipMemcpy (p->d_classlut, lut.data (), 65536 * 2, hipMemcpyHostToDevice) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    HIP_TRY (hipFuncSetAttribute (reinterpret_cast<const void *> (&classmap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 65536 * 2));
  }
  return ACM_GPU_OK;
}

/* kw_base: added to every keyword id the plan reports (the delta plans of acm_gpu_plan_update) */
int
plan_create (const ACMFlat *flat, int device, uint32_t kw_base, ACMPlan **out) {
  if (!flat || !out)
    return ACM_GPU_E_ARG;
  hipDeviceProp_t prop;
  int rc = device_properties (device, &prop);
  if (rc)
    return rc;
  PlanBuild B{};
  B.flat = flat;
  acm_flat_info (flat, &B.fi);
  acm_flat_view (flat, &B.fv);
  B.lds_cap = (uint32_t)prop.maxSharedMemoryPerMultiProcessor >= 160 * 1024 ? 160 * 1024 : 64 * 1024;
  B.kw_base = kw_base;
  if (B.fi.lmax >= (1u << 24))
    return ACM_GPU_E_INELIGIBLE;
  const bool interned = B.fi.sym_bytes == 8;
  if (interned) {
    if (!B.fv.keys64 && B.fi.n_edges)
      return ACM_GPU_E_ARG;
    B.fi.sym_bytes = 4; /* from here on: a machine over 4-byte ids */
  }

  ACMPlan *p = new (std::nothrow) ACMPlan ();
  if (!p)
    return ACM_GPU_E_NOMEM;
  p->device = device;
  p->finfo = B.fi;
  p->kw_base = kw_base;
  p->covered_keywords = B.fi.n_keywords;
  p->text_sym_bytes = interned ? 8 : B.fi.sym_bytes;
  p->cu_count = prop.multiProcessorCount;
  if (B.sw.segment_log2 >= 12 && B.sw.segment_log2 <= 31)
    p->segment = 1ull << B.sw.segment_log2;
  /* tests: fewer workgroups than CUs, so that one wave sees many tiles of a small text (the
   * overflow path of the item regions fires hundreds of times per wave) */
  if (B.sw.grid_blocks >= 1 && B.sw.grid_blocks < p->cu_count)
    p->cu_count = B.sw.grid_blocks;
  rc = build_tables (B, p);
  if (!rc)
    rc = set_lds_attributes (p);
  if (!rc)
    rc = build_text_side (p, B, interned);
  if (rc) {
    acm_gpu_plan_destroy (p); /* (takes a plan built part of the way) */
    return rc;
  }
  *out = p;
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_plan_create_flat (const ACMFlat *flat, int device, ACMPlan **out) {
  return plan_create (flat, device, 0, out);
}

extern "C" int
acm_gpu_plan_create (ACMachine *machine, int device, ACMPlan **out) {
  ACMFlat *flat = nullptr;
  int rc = acm_flatten (machine, &flat);
  if (rc)
    return rc;
  rc = acm_gpu_plan_create_flat (flat, device, out);
  acm_flat_release (flat);
  return rc;
}

extern "C" int
acm_gpu_plan_create_classes (ACMachine *machine, uint32_t sym_bytes, int device, ACMPlan **out) {
  ACMFlat *flat = nullptr;
  int rc = acm_flatten_classes (machine, sym_bytes, &flat);
  if (rc)
    return rc;
  rc = acm_gpu_plan_create_flat (flat, device, out);
  acm_flat_release (flat);
  if (!rc) {
    (*out)->class_sym_bytes = sym_bytes;
    if ((*out)->cls32) /* symbols a text brings are classified with the machine's own comparator */
      acm_internal_comparator (machine, &(*out)->cmp32, &(*out)->cmp32_arg);
  }
  return rc;
}

extern "C" void
acm_gpu_plan_destroy (ACMPlan *plan) {
  if (!plan)
    return;
  (void)hipSetDevice (plan->device);
  if (plan->delta || !plan->retired.empty ())
    (void)hipDeviceSynchronize (); /* scans with a retired delta may still be in flight */
  for (auto &r : plan->retired) {
    if (r.done)
      (void)hipEventDestroy (r.done);
    acm_gpu_plan_destroy (r.plan);
  }
  plan->retired.clear ();
  if (plan->delta)
    acm_gpu_plan_destroy (plan->delta);
  plan->delta = nullptr;
  for (auto &ev : plan->events) {
    (void)hipEventDestroy (ev.start);
    (void)hipEventDestroy (ev.scan_done);
    (void)hipEventDestroy (ev.all_done);
  }
  /* the device allocations of the plan's own (a delta's item buffer is its owner's) */
  void *const owned[] = { plan->blob, plan->own_items.items, plan->own_items.fill, plan->scratch.d_holes, plan->scratch.d_spill, plan->scratch.d_total,
                          plan->scratch.d_remap, plan->d_intern, plan->d_cls32, plan->d_unknown, plan->d_classlut };
  for (void *d : owned)
    if (d)
      (void)hipFree (d);
  if (plan->mir) {
    if (plan->mir->own)
      for (int t = 0; t < 5; t++)
        if (t != PT_LUT && plan->mir->dev[t])
          (void)hipFree (plan->mir->dev[t]);
    if (plan->mir->d_patches)
      (void)hipFree (plan->mir->d_patches);
    delete plan->mir;
  }
  delete plan;
}

extern "C" void
acm_gpu_plan_info (const ACMPlan *plan, ACMPlanInfo *info) {
  *info = plan->info;
  info->delta_keywords = plan->delta ? plan->delta->finfo.n_keywords : 0;
  info->merges = plan->merges;
  const bool gram = plan->kind == PlanKind::Gram;
  info->records_direct = ((gram && !plan->hashed) || plan->kind == PlanKind::Csr) ? 1u : 0u;
  info->variant = gram ? (plan->gram2 ? 2u : 0u) | (plan->short_pass ? 4u : 0u) | (plan->short_pass && !plan->short_ids_lds ? 8u : 0u) : 0u;
}

extern "C" int
acm_gpu_plan_status (ACMPlan *plan) {
  if (!plan)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  HIP_TRY (hipDeviceSynchronize ());
  if (!plan->scratch.d_total)
    return ACM_GPU_OK;
  unsigned int words[4] = { 0, 0, 0, 0 };
  HIP_TRY (hipMemcpy (words, plan->scratch.d_total, sizeof words, hipMemcpyDeviceToHost));
  if (words[3])
    return ACM_GPU_E_INTERNAL;
  return plan->delta ? acm_gpu_plan_status (plan->delta) : ACM_GPU_OK;
}

extern "C" int
acm_gpu_plan_timing (ACMPlan *plan, int enable) {
  if (!plan)
    return ACM_GPU_E_ARG;
  plan->timing = enable != 0;
  plan->timing_every = enable > 1 ? (uint32_t)enable : 1u;
  plan->timing_seq = 0;
  plan->events_used = 0;
  plan->timing_ms = 0;
  plan->timing_all_ms = 0;
  plan->timing_launches = 0;
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_plan_timing_read_all (ACMPlan *plan, double *scan_ms, double *all_ms, uint64_t *launches) {
  if (!plan)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  for (size_t i = 0; i < plan->events_used; i++) {
    HIP_TRY (hipEventSynchronize (plan->events[i].all_done));
    float ms = 0;
    HIP_TRY (hipEventElapsedTime (&ms, plan->events[i].start, plan->events[i].scan_done));
    plan->timing_ms += ms;
    HIP_TRY (hipEventElapsedTime (&ms, plan->events[i].start, plan->events[i].all_done));
    plan->timing_all_ms += ms;
    plan->timing_launches++;
  }
  plan->events_used = 0;
  if (scan_ms)
    *scan_ms = plan->timing_ms;
  if (all_ms)
    *all_ms = plan->timing_all_ms;
  if (launches)
    *launches = plan->timing_launches;
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_plan_timing_read (ACMPlan *plan, double *total_ms, uint64_t *launches) {
  return acm_gpu_plan_timing_read_all (plan, total_ms, nullptr, launches);
}

namespace {

int
timing_begin (ACMPlan *p, hipStream_t st, hipEvent_t *stop, hipEvent_t *stop_all) {
  *stop = nullptr;
  *stop_all = nullptr;
  if (!p->timing || p->timing_seq++ % p->timing_every != 0)
    return ACM_GPU_OK;
  if (p->events_used == p->events.size ()) {
    if (p->events.size () >= 4096) { /* fold what is recorded so far */
      int rc = acm_gpu_plan_timing_read (p, nullptr, nullptr);
      if (rc)
        return rc;
    } else {
      ACMPlan::LaunchEvents ev;
      HIP_TRY (hipEventCreate (&ev.start));
      HIP_TRY (hipEventCreate (&ev.scan_done));
      HIP_TRY (hipEventCreate (&ev.all_done));
      p->events.push_back (ev);
    }
  }
  auto &ev = p->events[p->events_used++];
  HIP_TRY (hipEventRecord (ev.start, st));
  *stop = ev.scan_done;
  *stop_all = ev.all_done;
  return ACM_GPU_OK;
}

template <bool COUNT_ONLY>
int
launch_sparse (ACMPlan *p, const EmitCtx &E, Launch a, hipStream_t st) {
  const uint32_t tps = 128 / p->finfo.sym_bytes;
  const uint32_t nsubs = (uint32_t)(((uint64_t)a.n + tps - 1) / tps);
  uint32_t grid = p->info.grid_blocks;
  const uint64_t lane_streams = (uint64_t)grid * (SPARSE_THREADS / WAVE) * WAVE * SPARSE_S;
  /* sub-chunks per chunk: about four tiles per wave, the warm-up at most a quarter of a chunk */
  uint64_t R = nsubs / (lane_streams * 4);
  const uint64_t rmin = 4ull * p->SK.warm_subs > 4 ? 4ull * p->SK.warm_subs : 4;
  if (R < rmin)
    R = rmin;
  if (R > 64 && R > rmin)
    R = 64 > rmin ? 64 : rmin;
  SparseK K = p->SK;
  K.R = (uint32_t)R;
  a.range_begin = 0;
  a.range_end = (uint32_t)((nsubs + R - 1) / R);
  const uint32_t tiles = (a.range_end + WAVE * SPARSE_S - 1) / (WAVE * SPARSE_S);
  const uint32_t wpb = SPARSE_THREADS / WAVE;
  if ((tiles + wpb - 1) / wpb < grid)
    grid = (tiles + wpb - 1) / wpb;
  void *args[] = { &K, const_cast<EmitCtx *> (&E), &a, &a.text };
  HIP_TRY (hipLaunchKernel (sparse_kernel (p, COUNT_ONLY), dim3 (grid),
                            dim3 (SPARSE_THREADS), args, p->sparse_lds_bytes, st));
  return ACM_GPU_OK;
}

/* the last sixteenth of the tiles [range_begin, range_end) becomes the dynamic pool (none for
 * launches of a few tiles per wave); counters alternate from launch to launch (TileShare) */
void
set_tile_pool (ACMPlan *p, Launch &a, uint32_t waves) {
  const uint32_t tiles = a.range_end - a.range_begin;
  const uint32_t pool = tiles >= waves * 8 ? tiles / 16 : 0;
  a.static_end = a.range_end - pool;
  const uint32_t blocks = waves / (SPARSE_THREADS / WAVE) > 0 ? waves / (SPARSE_THREADS / WAVE) : 1;
  a.pool_classes = blocks < POOL_CLASSES ? blocks : POOL_CLASSES; /* (grids of fewer blocks than parts: every part must have a block) */
  a.pool_class_tiles = (pool + a.pool_classes - 1) / a.pool_classes;
  a.pool_ctr = p->scratch.d_pool_ctr + (p->scratch.launch_seq & 1) * POOL_CLASSES * POOL_CTR_STRIDE;
  a.pool_reset = p->scratch.d_pool_ctr + ((p->scratch.launch_seq & 1) ^ 1) * POOL_CLASSES * POOL_CTR_STRIDE;
  p->scratch.launch_seq++;
}

/* records of the hits parked by `regions_used` waves of the start-parallel / 4-gram kernels */
void
launch_expand_hits (ACMPlan *p, const EmitCtx &E, uint32_t regions_used, hipStream_t st) {
  /* 1024 threads per 16 regions (config 3, 4 GiB: 1.10 ms; 8, 4, 2 regions or smaller blocks: 1.25-1.33) */
  const ItemBuffer &I = p->items ();
  hipLaunchKernelGGL ((expand_hits_kernel<1024, 16>), dim3 ((regions_used + 15) / 16), dim3 (1024), 0, st, E,
                      static_cast<const uint2 *> (I.items), I.region_items, I.fill, regions_used);
}

/* The tiles of one launch of a start-parallel kernel (scan_starts, scan_gram / gram2, scan_short)
 * over a segment of n symbols: tile t is the groups [t * R, (t + 1) * R) of `group` symbols each,
 * the launch takes the tiles [begin, end) with `grid` blocks.
 *   back    a match that ends at emit_from or later starts no earlier than emit_from - back: the
 *           groups in front of that one are skipped
 *   blocks  the blocks of a full grid: R = groups to scan / (16 tiles for each of their waves),
 *           within 4 .. 64 (4 to 64 KiB of text a tile); fewer blocks than that when there are few tiles
 *   round4  R a multiple of 4 (kernels that take a tile's groups four at a time)
 *   fixed_R not 0: R whatever the text (experiments) */
struct TileGeometry {
  uint32_t R, begin, end, grid;
};
constexpr uint32_t TILE_R_MIN = 4, TILE_R_MAX = 64;
TileGeometry
tile_geometry (uint32_t n, uint32_t emit_from, uint32_t group, uint32_t back, uint32_t blocks, bool round4, uint32_t fixed_R = 0) {
  const uint32_t wpb = SPARSE_THREADS / WAVE;
  const uint32_t ngroups = (uint32_t)(((uint64_t)n + group - 1) / group);
  const uint32_t first_group = (emit_from > back ? emit_from - back : 0) / group;
  uint64_t R = (ngroups - first_group) / ((uint64_t)blocks * wpb * 16);
  if (round4)
    R &= ~3ull;
  R = R < TILE_R_MIN ? TILE_R_MIN : (R > TILE_R_MAX ? TILE_R_MAX : R);
  if (fixed_R)
    R = fixed_R;
  TileGeometry T;
  T.R = (uint32_t)R;
  T.begin = first_group / T.R;
  T.end = (uint32_t)((ngroups + R - 1) / R);
  const uint32_t tiles = T.end - T.begin;
  T.grid = (tiles + wpb - 1) / wpb < blocks ? (tiles + wpb - 1) / wpb : blocks;
  return T;
}

/* a match that ends at emit_from or later starts no earlier than emit_from - (lmax - 1) */
uint32_t
lookback (const ACMPlan *p) {
  return p->finfo.lmax > 1 ? p->finfo.lmax - 1 : 0;
}

template <bool COUNT_ONLY>
int
launch_starts (ACMPlan *p, const EmitCtx &E, Launch a, hipStream_t st, hipEvent_t stop) {
  const uint32_t wpb = SPARSE_THREADS / WAVE;
  /* groups of 1 KiB; about sixteen tiles per wave, 4 to 64 KiB each, a multiple of 4 */
  const TileGeometry T = tile_geometry (a.n, a.emit_from, WAVE * (16 / p->finfo.sym_bytes), lookback (p), p->info.grid_blocks, true);
  StartsK K = p->TK;
  K.R = T.R;
  a.range_begin = T.begin;
  a.range_end = T.end;
  set_tile_pool (p, a, T.grid * wpb);
  ItemBuffer &I = p->items ();
  void *items = COUNT_ONLY ? nullptr : I.items;
  uint32_t *fill = COUNT_ONLY ? nullptr : I.fill;
  void *args[] = { &K, const_cast<EmitCtx *> (&E), &a, &a.text, &items, &I.region_items, &fill };
  HIP_TRY (hipLaunchKernel (starts_kernel (p, COUNT_ONLY), dim3 (T.grid), dim3 (SPARSE_THREADS), args, p->starts_lds_bytes, st));
  if (stop) /* the timing brackets the scan kernel alone, as for the dense kernel */
    HIP_TRY (hipEventRecord (stop, st));
  if (!COUNT_ONLY)
    launch_expand_hits (p, E, T.grid * wpb, st);
  return ACM_GPU_OK;
}

/* the tiles of one launch of the 4-gram kernel over a segment of n symbols: groups of 1,024
 * symbols, one block a CU, R as it comes (any number of groups; tiled_layout's bound counts on
 * GRAM_R_MIN) */
constexpr uint32_t GRAM_R_MIN = TILE_R_MIN;
TileGeometry
gram_tiling (const ACMPlan *p, uint32_t n, uint32_t emit_from) {
  static const int r_env = getenv ("ACM_GPU_GRAM_R") ? atoi (getenv ("ACM_GPU_GRAM_R")) : 0; /* experiments: groups per tile (a multiple of 4, up to 64) */
  const uint32_t fixed_R = (r_env >= 4 && r_env <= 64 && r_env % 4 == 0) ? (uint32_t)r_env : 0;
  return tile_geometry (n, emit_from, WAVE * 16, lookback (p), (uint32_t)p->cu_count, false, fixed_R);
}

/* ACM_GPU_CLOSE_SORT=network: close_holes_kernel sorts its descriptors with the bitonic network whatever
 * their spread (its fallback for crowded buckets; tests) */
uint32_t
close_network_only () {
  const char *e = getenv ("ACM_GPU_CLOSE_SORT");
  return e && strcmp (e, "network") == 0 ? 1u : 0u;
}

/* the holes the `n_waves` waves of a pass left in their last chunks of records (the waves of the
 * scan's widest launch: an earlier segment may have had more blocks than the last one; a short text
 * has few -- every block of the kernel sorts all the descriptors it is given) */
hipError_t
launch_close_holes (ACMPlan *p, const EmitCtx &E, const RecHole *holes, uint32_t n_waves, hipStream_t st) {
  uint32_t npow = 64;
  while (npow < n_waves)
    npow <<= 1;
  const uint32_t blocks = n_waves / 16 > 0 ? n_waves / 16 : 1; /* 16 holes per block */
  hipLaunchKernelGGL (close_holes_kernel, dim3 (blocks), dim3 (CLOSE_THREADS), npow * 16, st, E, holes, n_waves, npow,
                      reinterpret_cast<unsigned int *> (p->scratch.d_total + 1), close_network_only ());
  return hipGetLastError ();
}

/* a tiled scan in progress (acm_gpu_scan_ordered_device -> scan_tiled): the 4-gram kernel writes a
 * TileEntry per tile from dir[base] on and links its chunks in chunk_prev */
struct TiledScan {
  TileEntry *dir;
  uint32_t *chunk_prev;
  uint32_t base; /* tiles of the launches so far */
};

/* holes_waves: waves of the widest launch of the scan at hand so far -- the holes to close behind its
 * last segment; tiled: the scan is a tiled one (narrow alphabets, record mode) */
template <bool COUNT_ONLY>
int
launch_gram (ACMPlan *p, const EmitCtx &E, Launch a, hipStream_t st, hipEvent_t stop, bool first_segment, bool last_segment,
             uint32_t &holes_waves, TiledScan *tiled) {
  const uint32_t wpb = SPARSE_THREADS / WAVE;
  const TileGeometry T = gram_tiling (p, a.n, a.emit_from);
  const uint32_t grid = T.grid, tiles = T.end - T.begin;
  GramK K = p->GK;
  K.R = T.R;
  a.range_begin = T.begin;
  a.range_end = T.end;
  set_tile_pool (p, a, grid * wpb);
  /* narrow alphabets: the kernel writes the records itself (no item buffer, no expansion; the holes
   * its waves leave in their last chunks are closed right behind it); hashed windows: hits parked
   * per wave and expanded as in the start-parallel kernel */
  const bool direct = !p->hashed;
  ItemBuffer &I = p->items ();
  void *items = (COUNT_ONLY || direct) ? nullptr : I.items;
  uint32_t *fill = (COUNT_ONLY || direct) ? nullptr : I.fill;
  void *holes = (!COUNT_ONLY && direct) ? p->scratch.d_holes : nullptr;
  /* the segments of one scan share the waves' chunks of records: a wave picks up in segment k + 1
   * the chunk it was filling at the end of segment k (its hole descriptor says where), and the
   * holes are closed once, behind the last segment */
  uint32_t resume = first_segment ? 0u : 1u;
  if (holes && first_segment)
    HIP_TRY (hipMemsetAsync (holes, 0, (size_t)p->scratch.direct_regions * sizeof (RecHole), st));
  if (first_segment || grid * wpb > holes_waves)
    holes_waves = grid * wpb;
  /* a tiled scan: a directory entry per tile, the chunks linked, the holes left alone (dev_tiles.h) */
  TileEntry *dir = tiled ? tiled->dir : nullptr;
  uint32_t dir_base = tiled ? tiled->base : 0;
  if (tiled)
    tiled->base += tiles;
  void *args[] = { &K, const_cast<EmitCtx *> (&E), &a, &a.text, &items, &I.region_items, &fill, &holes, &resume, &dir, &dir_base };
  HIP_TRY (hipLaunchKernel (gram_kernel (p, COUNT_ONLY, tiled != nullptr), dim3 (grid), dim3 (SPARSE_THREADS), args, p->gram_lds_bytes, st));
  if (stop)
    HIP_TRY (hipEventRecord (stop, st));
  if (!COUNT_ONLY) {
    if (direct && tiled) {
      /* (nothing: tile_gather_kernel reads the records where they lie) */
    } else if (direct && last_segment) {
      HIP_TRY (launch_close_holes (p, E, static_cast<const RecHole *> (p->scratch.d_holes), holes_waves, st));
    } else if (!direct)
      launch_expand_hits (p, E, grid * wpb, st);
  }
  return ACM_GPU_OK;
}

/* the keywords of 1-3 symbols of a 4-gram plan over a narrow alphabet: a pass of their own over the
 * segment (dev_short.h), into the same record buffer; its waves' holes have descriptors of their own */
template <bool COUNT_ONLY>
int
launch_short (ACMPlan *p, const EmitCtx &E, Launch a, hipStream_t st, hipEvent_t stop, bool first_segment, bool last_segment,
              uint32_t &holes_waves) {
  const uint32_t wpb = SPARSE_THREADS / WAVE;
  const uint32_t short_regions = p->scratch.direct_regions;
  /* (count-only: 61 registers, two blocks a CU while LDS allows; with records one.)  A match of 1-3
   * symbols that ends at emit_from or later starts no earlier than emit_from - 2; R a multiple of
   * 4: the kernel takes a tile's groups four at a time */
  const TileGeometry T = tile_geometry (a.n, a.emit_from, WAVE * 16, 2, (uint32_t)p->cu_count * (COUNT_ONLY ? p->short_blocks_per_cu : 1u), true);
  const uint32_t grid = T.grid;
  GramK K = p->GK;
  K.R = T.R;
  a.range_begin = T.begin;
  a.range_end = T.end;
  set_tile_pool (p, a, grid * wpb);
  RecHole *holes = COUNT_ONLY ? nullptr : static_cast<RecHole *> (p->scratch.d_holes) + p->scratch.direct_regions;
  uint32_t resume = first_segment ? 0u : 1u;
  if (holes && first_segment)
    HIP_TRY (hipMemsetAsync (holes, 0, (size_t)short_regions * sizeof (RecHole), st));
  if (first_segment || grid * wpb > holes_waves)
    holes_waves = grid * wpb;
  void *args[] = { &K, const_cast<EmitCtx *> (&E), &a, &a.text, &holes, &resume };
  HIP_TRY (hipLaunchKernel (short_kernel (p, COUNT_ONLY), dim3 (grid), dim3 (SPARSE_THREADS), args,
                            COUNT_ONLY ? p->short_lds_count_bytes : p->short_lds_bytes, st));
  if (stop)
    HIP_TRY (hipEventRecord (stop, st));
  if (!COUNT_ONLY && last_segment)
    HIP_TRY (launch_close_holes (p, E, holes, holes_waves, st));
  return ACM_GPU_OK;
}

template <bool COUNT_ONLY>
int
launch_csr (ACMPlan *p, const EmitCtx &E, Launch a, hipStream_t st) {
  if (a.range_end <= a.range_begin)
    return ACM_GPU_OK;
  const uint64_t len = a.range_end - a.range_begin;
  /* chunk length: enough chunks to fill the chip, long enough to amortise the warm-up */
  const uint64_t target_lanes = (uint64_t)p->cu_count * 16 * WAVE;
  uint64_t chunk = (len + target_lanes - 1) / target_lanes;
  const uint64_t minchunk = 64 > 8ull * p->finfo.lmax ? 64 : 8ull * p->finfo.lmax;
  if (chunk < minchunk)
    chunk = minchunk;
  if (chunk > 4096 && chunk > minchunk)
    chunk = 4096 > minchunk ? 4096 : minchunk;
  const uint64_t nchunks = (len + chunk - 1) / chunk;
  uint64_t blocks = (nchunks + WAVE - 1) / WAVE;
  const uint64_t maxblocks = (uint64_t)p->cu_count * 32;
  if (blocks > maxblocks)
    blocks = maxblocks;
  dim3 g ((uint32_t)blocks), b (WAVE);
  switch (p->finfo.sym_bytes) {
  case 1: hipLaunchKernelGGL ((scan_csr_kernel<uint8_t, COUNT_ONLY>), g, b, 0, st, p->csr, E, a, (uint32_t)chunk); break;
  case 2: hipLaunchKernelGGL ((scan_csr_kernel<uint16_t, COUNT_ONLY>), g, b, 0, st, p->csr, E, a, (uint32_t)chunk); break;
  default: hipLaunchKernelGGL ((scan_csr_kernel<uint32_t, COUNT_ONLY>), g, b, 0, st, p->csr, E, a, (uint32_t)chunk); break;
  }
  HIP_TRY (hipGetLastError ());
  return ACM_GPU_OK;
}

/* (re)allocate the item buffer for segments of up to n symbols: room for one item per 256
 * symbols, at least 256 per wave; denser matches are expanded in the kernel itself */
int
ensure_item_buffer (ACMPlan *user, uint64_t n, uint32_t symbols_per_item = 256, uint32_t min_items = 256) {
  /* a delta plan parks in the buffer of the plan it belongs to: their scans run one after the
   * other on one stream, and a fresh 140 MB buffer (with the waits it takes to set one up) for
   * every delta made every dictionary change cost more than the delta itself */
  ItemBuffer *buf = &user->items ();
  /* one region per wave of the kernels that park items (dense, 4-gram, start-parallel: one block of
   * 16 waves per CU) -- of the plan that SCANS, not of the buffer's owner: an owner of the CSR kind
   * (a plan made from an empty machine) has cu_count * 16 single-wave blocks, which sized the
   * buffer of a dense delta at 65,536 regions x 4,352 items = 2.3 GB */
  uint32_t regions = (uint32_t)user->cu_count * (DENSE_THREADS / WAVE);
  if (buf->items && buf->regions > regions)
    regions = buf->regions; /* (shared by a plan and its delta: never shrink what the other one uses) */
  uint64_t per = (n / symbols_per_item + regions - 1) / regions;
  per = (per + 63) / 64 * 64;
  if (per < min_items)
    per = min_items;
  if (per > (1u << 20))
    per = 1u << 20;
  if (!(buf->items && buf->regions == regions && buf->region_items >= per)) {
    if (buf->items || buf->fill)
      HIP_TRY (hipDeviceSynchronize ()); /* earlier scans (pieces of a stream) may still be parking items */
    if (buf->items)
      HIP_TRY (hipFree (buf->items));
    if (buf->fill)
      HIP_TRY (hipFree (buf->fill));
    buf->items = nullptr;
    buf->fill = nullptr;
    if (hipMalloc (&buf->items, (size_t)regions * per * 8) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    if (hipMalloc (reinterpret_cast<void **> (&buf->fill), (size_t)regions * 4) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    HIP_TRY (hipMemset (buf->fill, 0, (size_t)regions * 4));
    /* the memset runs on the null stream; the scans may run on streams that do not wait for it */
    HIP_TRY (hipDeviceSynchronize ());
    buf->regions = regions;
    buf->region_items = (uint32_t)per;
  }
  return ACM_GPU_OK;
}

/* hole descriptors and spill area of a plan whose scan kernel writes the records itself */
int
ensure_direct_buffers (ACMPlan *p, uint32_t rec_chunk) {
  const uint32_t regions = (uint32_t)p->cu_count * (SPARSE_THREADS / WAVE);
  if (p->scratch.d_holes && p->scratch.d_spill && p->scratch.direct_regions >= regions && p->scratch.spill_chunk >= rec_chunk)
    return ACM_GPU_OK;
  if (p->scratch.d_holes || p->scratch.d_spill)
    HIP_TRY (hipDeviceSynchronize ());
  if (p->scratch.d_holes)
    HIP_TRY (hipFree (p->scratch.d_holes));
  if (p->scratch.d_spill)
    HIP_TRY (hipFree (p->scratch.d_spill));
  p->scratch.d_holes = p->scratch.d_spill = nullptr;
  if (hipMalloc (&p->scratch.d_holes, (size_t)regions * 2 * sizeof (RecHole)) != hipSuccess || /* (the 4-gram pass's and the short-keyword pass's) */
      hipMalloc (&p->scratch.d_spill, (size_t)regions * rec_chunk * 16) != hipSuccess) /* (one chunk per wave: 64 MB, 256 MB with big chunks) */
    return ACM_GPU_E_NOMEM;
  p->scratch.direct_regions = regions;
  p->scratch.spill_chunk = rec_chunk;
  return ACM_GPU_OK;
}

/* expand_items_once_kernel: 1024 threads per 16 regions (one block per CU on config 2), the items
 * of 4 rounds in registers, one atomic per block (measured against one atomic per round of 1,024
 * items, smaller blocks and fewer rounds: DESIGN.md 4.2) */
template <bool CONT, bool COUNT_ONLY>
void
launch_expand_cfg (ACMPlan *p, const EmitCtx &E, uint32_t regions_used, const ExpandTail &tail, hipStream_t st) {
  const dim3 g ((regions_used + 15) / 16);
  const ItemBuffer &I = p->items ();
  hipLaunchKernelGGL ((expand_items_once_kernel<CONT, COUNT_ONLY, 1024, 16, 4>), g, dim3 (1024), 0, st, E,
                      static_cast<const uint2 *> (I.items), I.region_items, I.fill, tail);
}

/* scan kernel, then the expansion of what it parked; the caller's counter is written by the
 * expansion of the last segment (no memsets: both kernels leave their bookkeeping zeroed) */
template <bool COUNT_ONLY>
int
launch_dense (ACMPlan *p, const EmitCtx &E, Launch a, hipStream_t st, hipEvent_t stop, uint64_t *d_count, bool last_segment) {
  const uint32_t TILE = WAVE * p->streams * p->chunk;
  a.range_begin = 0;
  a.range_end = (uint32_t)(((uint64_t)a.n + TILE - 1) / TILE);
  uint32_t grid = p->info.grid_blocks;
  const uint32_t wpb = DENSE_THREADS / WAVE;
  const uint32_t blocks_needed = (a.range_end + wpb - 1) / wpb;
  if (blocks_needed < grid)
    grid = blocks_needed;
  static_assert (DENSE_THREADS == SPARSE_THREADS, "set_tile_pool counts blocks of SPARSE_THREADS");
  set_tile_pool (p, a, grid * wpb);
  ItemBuffer &I = p->items ();
  void *args[] = { &p->K, const_cast<EmitCtx *> (&E), &a, &p->d_dense, &p->d_lds_image, &p->lds_image_bytes, &a.text,
                   &I.items, &I.region_items, &I.fill, &p->d_dstart };
  HIP_TRY (hipLaunchKernel (dense_kernel (p, COUNT_ONLY), dim3 (grid), dim3 (DENSE_THREADS), args, p->dense_lds_launch, st));
  if (stop)
    HIP_TRY (hipEventRecord (stop, st));
  ExpandTail tail;
  tail.user_count = reinterpret_cast<unsigned long long *> (d_count);
  tail.ticket = reinterpret_cast<unsigned int *> (p->scratch.d_total + 1);
  tail.last_segment = last_segment ? 1 : 0;
  if (p->entry_bytes == 2)
    launch_expand_cfg<true, COUNT_ONLY> (p, E, grid * wpb, tail, st);
  else
    launch_expand_cfg<false, COUNT_ONLY> (p, E, grid * wpb, tail, st);
  HIP_TRY (hipGetLastError ());
  return ACM_GPU_OK;
}

/* ---- incremental updates of a start-parallel plan */
/* brings the device tables in line with the mirror, on the stream of the scan that follows */
int
starts_flush (ACMPlan *p, hipStream_t st) {
  StartsMirror &M = *p->mir;
  if (M.full_upload) {
    /* (re)allocate with headroom and send everything; scans already enqueued still read the
     * old arrays, so wait for them before those are freed */
    HIP_TRY (hipDeviceSynchronize ());
    uint32_t *fresh[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    size_t want[5];
    for (int t = 0; t < 5; t++) {
      if (t == PT_LUT)
        continue; /* fixed size, stays in the plan's blob */
      want[t] = M.tab[t].size () * 2 + 4096;
      const bool keep = M.own && M.cap[t] >= M.tab[t].size ();
      if (keep)
        fresh[t] = M.dev[t];
      else if (hipMalloc (reinterpret_cast<void **> (&fresh[t]), want[t] * 4) != hipSuccess ||
               hipMemset (fresh[t], 0, want[t] * 4) != hipSuccess) { /* words never set are 0 in the mirror too */
        for (int u = 0; u <= t; u++)
          if (fresh[u] && fresh[u] != M.dev[u])
            (void)hipFree (fresh[u]);
        return ACM_GPU_E_NOMEM;
      }
    }
    for (int t = 0; t < 5; t++) {
      if (t == PT_LUT) {
        HIP_TRY (hipMemcpy (M.dev[t], M.tab[t].data (), M.tab[t].size () * 4, hipMemcpyHostToDevice));
        continue;
      }
      HIP_TRY (hipMemcpy (fresh[t], M.tab[t].data (), M.tab[t].size () * 4, hipMemcpyHostToDevice));
      if (fresh[t] != M.dev[t]) {
        if (M.own && M.dev[t])
          HIP_TRY (hipFree (M.dev[t]));
        M.dev[t] = fresh[t];
        M.cap[t] = want[t];
      }
    }
    M.own = true;
    M.full_upload = false;
    M.patches.clear ();
    p->TK.srec = reinterpret_cast<const uint4 *> (M.dev[PT_REC]);
    p->TK.sedge = reinterpret_cast<const uint2 *> (M.dev[PT_EDGE]);
    p->TK.pairs = reinterpret_cast<const uint2 *> (M.dev[PT_PAIRS]);
    p->d_oinfo = reinterpret_cast<const uint4 *> (M.dev[PT_OINFO]);
    return ACM_GPU_OK;
  }
  if (M.patches.empty ())
    return ACM_GPU_OK;
  /* a word may have been set several times since the last flush and the patch kernel writes in
   * no particular order: every patch carries the word's final value */
  for (uint4 &q : M.patches)
    q.z = M.tab[q.x][q.y];
  const size_t np = M.patches.size ();
  if (M.cap_patches < np) {
    if (M.d_patches) {
      HIP_TRY (hipStreamSynchronize (st));
      HIP_TRY (hipFree (M.d_patches));
      M.d_patches = nullptr;
    }
    M.cap_patches = np * 2 + 1024;
    if (hipMalloc (reinterpret_cast<void **> (&M.d_patches), M.cap_patches * sizeof (uint4)) != hipSuccess) {
      M.cap_patches = 0;
      return ACM_GPU_E_NOMEM;
    }
  }
  /* (blocking copy ordered on the stream: the staging vector can be reused at once, and an
   * earlier patch kernel that reads d_patches has finished before it is overwritten) */
  HIP_TRY (hipMemcpyWithStream (M.d_patches, M.patches.data (), np * sizeof (uint4), hipMemcpyHostToDevice, st));
  PatchTables T;
  for (int t = 0; t < 5; t++)
    T.t[t] = M.dev[t];
  HIP_TRY (launch (patch_kernel, dim3 ((uint32_t)((np + 255) / 256)), dim3 (256), 0, st, T, M.d_patches, (uint32_t)np));
  M.patches.clear ();
  return ACM_GPU_OK;
}

/* goto edge of mirror state s on symbol c (NONE if there is none) */
uint32_t
mirror_child (const StartsMirror &M, uint32_t s, uint32_t c) {
  const uint32_t *r = &M.tab[PT_REC][8 * (size_t)s];
  const uint32_t ne = r[1];
  if (s == 0 && c < M.tab[PT_LUT].size ()) /* the root table answers for the symbols it holds */
    return (M.tab[PT_LUT][c] & ST_STATE) ? (M.tab[PT_LUT][c] & ST_STATE) : NONE;
  if (ne <= 2 && s != 0) {
    if (ne >= 1 && r[4] == c)
      return r[5];
    if (ne >= 2 && r[6] == c)
      return r[7];
    return NONE;
  }
  uint32_t lo = r[2], hi = r[2] + ne;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (M.tab[PT_EDGE][2 * (size_t)mid] < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < r[2] + ne && M.tab[PT_EDGE][2 * (size_t)lo] == c ? M.tab[PT_EDGE][2 * (size_t)lo + 1] : NONE;
}

/* root-table entry of the root's child `child` (its flags follow from its record) */
void
mirror_refresh_root_child (StartsMirror &M, uint32_t child) {
  const uint32_t sym = M.parent_sym[child];
  const uint32_t *r = &M.tab[PT_REC][8 * (size_t)child];
  const uint32_t ne = r[1];
  const bool always = r[3] != 0 || ne > 2 || ne == 0;
  M.set (PT_PAIRS, 2 * (size_t)child, ne >= 1 ? r[4] : 0);
  M.set (PT_PAIRS, 2 * (size_t)child + 1, ne >= 2 ? r[6] : (ne >= 1 ? r[4] : 0));
  if (sym < M.tab[PT_LUT].size ())
    M.set (PT_LUT, sym, (M.tab[PT_LUT][sym] & ST_SECOND) | child | (always ? ST_ALWAYS : 0u));
}

/* adds the edge s --c--> nx: rows stay sorted; states with more than two edges (and the root)
 * keep theirs in the edge table, in a slot range with room to grow */
void
mirror_add_edge (StartsMirror &M, uint32_t s, uint32_t c, uint32_t nx) {
  if (s == 0 && c < M.tab[PT_LUT].size ()) { /* the root-table entry (mirror_refresh_root_child) is the edge */
    M.n_edges++;
    return;
  }
  const size_t R = 8 * (size_t)s;
  const uint32_t ne = M.tab[PT_REC][R + 1];
  std::vector<std::pair<uint32_t, uint32_t>> row;
  row.reserve (ne + 1);
  if (ne <= 2 && s != 0) {
    if (ne >= 1)
      row.emplace_back (M.tab[PT_REC][R + 4], M.tab[PT_REC][R + 5]);
    if (ne >= 2)
      row.emplace_back (M.tab[PT_REC][R + 6], M.tab[PT_REC][R + 7]);
  } else {
    const uint32_t b = M.tab[PT_REC][R + 2];
    for (uint32_t e = 0; e < ne; e++)
      row.emplace_back (M.tab[PT_EDGE][2 * (size_t)(b + e)], M.tab[PT_EDGE][2 * (size_t)(b + e) + 1]);
  }
  row.insert (std::upper_bound (row.begin (), row.end (), std::make_pair (c, 0u),
                                [] (const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) { return a.first < b.first; }),
              std::make_pair (c, nx));
  const uint32_t nn = ne + 1;
  if (nn > 2 || s == 0) {
    uint32_t begin = M.tab[PT_REC][R + 2], capacity = M.tab[PT_REC][R + 0];
    if (capacity < nn || (ne <= 2 && s != 0)) { /* no slots yet, or no room: a new range at the end */
      capacity = nn * 2 > 4 ? nn * 2 : 4;
      begin = (uint32_t)(M.tab[PT_EDGE].size () / 2);
      M.tab[PT_EDGE].resize ((size_t)(begin + capacity) * 2, 0);
      if ((size_t)(begin + capacity) * 2 > M.cap[PT_EDGE])
        M.full_upload = true;
      M.set (PT_REC, R + 0, capacity);
      M.set (PT_REC, R + 2, begin);
    }
    for (uint32_t e = 0; e < nn; e++) {
      M.set (PT_EDGE, 2 * (size_t)(begin + e), row[e].first);
      M.set (PT_EDGE, 2 * (size_t)(begin + e) + 1, row[e].second);
    }
  }
  M.set (PT_REC, R + 1, nn);
  M.set (PT_REC, R + 4, row[0].first);
  M.set (PT_REC, R + 5, row[0].second);
  M.set (PT_REC, R + 6, nn >= 2 ? row[1].first : 0);
  M.set (PT_REC, R + 7, nn >= 2 ? row[1].second : 0);
  M.n_edges++;
}

/* one new keyword: symbols[0 .. len), keyword id kw */
void
mirror_insert (StartsMirror &M, const uint32_t *symbols, uint32_t len, uint32_t kw) {
  uint32_t s = 0;
  for (uint32_t i = 0; i < len; i++) {
    const uint32_t c = symbols[i];
    uint32_t nx = mirror_child (M, s, c);
    if (nx == NONE) {
      nx = M.n_states++;
      M.parent.push_back (s);
      M.parent_sym.push_back (c);
      M.depth.push_back (i + 1);
      for (int w = 0; w < 8; w++)
        M.set (PT_REC, 8 * (size_t)nx + w, 0);
      if (M.tab[PT_REC].size () < 8 * (size_t)(nx + 1))
        M.tab[PT_REC].resize (8 * (size_t)(nx + 1), 0);
      if (M.tab[PT_PAIRS].size () < 2 * (size_t)(nx + 1))
        M.tab[PT_PAIRS].resize (2 * (size_t)(nx + 1), 0);
      if (M.tab[PT_OINFO].size () < 4 * (size_t)(nx + 1))
        M.tab[PT_OINFO].resize (4 * (size_t)(nx + 1), 0);
      if (8 * (size_t)(nx + 1) > M.cap[PT_REC] || 2 * (size_t)(nx + 1) > M.cap[PT_PAIRS] || 4 * (size_t)(nx + 1) > M.cap[PT_OINFO])
        M.full_upload = true;
      mirror_add_edge (M, s, c, nx);
      if (s == 0)
        mirror_refresh_root_child (M, nx); /* a new child of the root: its root-table entry */
      else if (M.parent[s] == 0 && s != 0) {
        /* s is a child of the root and got another edge: c is now a second symbol, and the
         * child's pair / ALWAYS flag may have changed */
        if (c < M.tab[PT_LUT].size ())
          M.set (PT_LUT, c, M.tab[PT_LUT][c] | ST_SECOND);
        mirror_refresh_root_child (M, s);
      }
    }
    s = nx;
  }
  /* terminal: what a record of this keyword carries (length, keyword id) */
  M.set (PT_REC, 8 * (size_t)s + 3, 1);
  M.set (PT_OINFO, 4 * (size_t)s + 0, 1);
  M.set (PT_OINFO, 4 * (size_t)s + 2, len);
  M.set (PT_OINFO, 4 * (size_t)s + 3, kw);
  if (M.parent[s] == 0 && s != 0)
    mirror_refresh_root_child (M, s);
  if (len > M.lmax)
    M.lmax = len;
  M.n_keywords++;
}

/* maps n symbols of d_text to class ids into the plan's own buffer (grown as needed) */
int
ensure_remap_buffer (ACMPlan *p, size_t bytes, hipStream_t st) {
  if (p->scratch.remap_bytes < bytes + 16) {
    if (p->scratch.d_remap) {
      HIP_TRY (hipStreamSynchronize (st)); /* an earlier scan may still read the old buffer */
      HIP_TRY (hipFree (p->scratch.d_remap));
      p->scratch.d_remap = nullptr;
      p->scratch.remap_bytes = 0;
    }
    const size_t want = bytes + bytes / 8 + 4096;
    if (hipMalloc (&p->scratch.d_remap, want) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    p->scratch.remap_bytes = want;
  }
  return ACM_GPU_OK;
}

int
classmap_text (ACMPlan *p, const void *d_text, uint64_t n, hipStream_t st) {
  const uint32_t sb = p->finfo.sym_bytes;
  const size_t bytes = (size_t)n * sb;
  int rc0 = ensure_remap_buffer (p, bytes, st);
  if (rc0)
    return rc0;
  const bool aligned = (reinterpret_cast<uintptr_t> (d_text) & 15) == 0;
  const uint64_t blocks16 = aligned ? bytes / 16 : 0;
  if (blocks16) {
    const uint64_t want_blocks = (blocks16 + 1023) / 1024;
    const uint32_t grid = (uint32_t)(want_blocks < (uint64_t)p->cu_count ? want_blocks : (uint64_t)p->cu_count);
    hipLaunchKernelGGL (classmap_kernel, dim3 (grid), dim3 (1024), 65536 * 2, st, static_cast<const uint4 *> (d_text),
                        static_cast<uint4 *> (p->scratch.d_remap), blocks16, p->d_classlut);
  }
  const uint64_t done = blocks16 * 16 / sb;
  if (done < n) {
    const uint64_t left = n - done;
    const uint32_t grid = (uint32_t)((left + 255) / 256 < 4096 ? (left + 255) / 256 : 4096);
    if (sb == 1)
      hipLaunchKernelGGL ((classmap_tail_kernel<uint8_t>), dim3 (grid), dim3 (256), 0, st, static_cast<const uint8_t *> (d_text),
                          static_cast<uint8_t *> (p->scratch.d_remap), done, n, p->d_classlut);
    else
      hipLaunchKernelGGL ((classmap_tail_kernel<uint16_t>), dim3 (grid), dim3 (256), 0, st, static_cast<const uint16_t *> (d_text),
                          static_cast<uint16_t *> (p->scratch.d_remap), done, n, p->d_classlut);
  }
  HIP_TRY (hipGetLastError ());
  return ACM_GPU_OK;
}

/* comparator classes of 4-byte symbols: class of a symbol the tables have not seen, by bisection
 * among the class representatives with the machine's comparator (0: equal to none of them) */
uint32_t
classify_symbol32 (const ACMPlan *p, uint32_t sym) {
  uint32_t lo = 0, hi = (uint32_t)p->cls32_reps.size ();
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const int c = p->cmp32 (&sym, &p->cls32_reps[mid], p->cmp32_arg);
    if (c == 0)
      return mid + 1;
    if (c < 0)
      hi = mid;
    else
      lo = mid + 1;
  }
  return 0;
}

/* the device table from everything classified so far (grown to stay at most a quarter full) */
int
upload_cls32_table (ACMPlan *p, hipStream_t st) {
  uint32_t slots = p->cls32_slots ? p->cls32_slots : 1u << 12;
  while ((uint64_t)slots < 4ull * (p->cls32_known.size () + p->cls32_cap))
    slots <<= 1;
  if (slots != p->cls32_slots) {
    if (p->d_cls32) {
      HIP_TRY (hipStreamSynchronize (st));
      HIP_TRY (hipFree (p->d_cls32));
      p->d_cls32 = nullptr;
    }
    if (hipMalloc (reinterpret_cast<void **> (&p->d_cls32), (size_t)slots * 8) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    p->cls32_slots = slots;
  }
  std::vector<unsigned long long> tab (slots, 0ull);
  auto mix = [] (uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
  };
  for (const auto &kv : p->cls32_known) {
    uint32_t h = (uint32_t)mix (kv.first) & (slots - 1);
    while (tab[h])
      h = (h + 1) & (slots - 1);
    tab[h] = ((unsigned long long)(kv.second + 1) << 32) | kv.first;
  }
  HIP_TRY (hipMemcpyWithStream (p->d_cls32, tab.data (), (size_t)slots * 8, hipMemcpyHostToDevice, st));
  p->cls32_uploaded = (uint32_t)p->cls32_known.size ();
  return ACM_GPU_OK;
}

/* maps n 4-byte symbols of d_text to class ids into the plan's own buffer.  Symbols the plan has
 * not met yet come back on a list, are classified here with the comparator and the pass is
 * repeated: the call waits for the stream (once when the text brings nothing new). */
int
classify_text32 (ACMPlan *p, const void *d_text, uint64_t n, hipStream_t st) {
  if (reinterpret_cast<uintptr_t> (d_text) & 3)
    return ACM_GPU_E_ARG;
  int rc = ensure_remap_buffer (p, (size_t)n * 4, st);
  if (rc)
    return rc;
  if (!p->d_cls32 || p->cls32_uploaded != p->cls32_known.size ()) {
    rc = upload_cls32_table (p, st);
    if (rc)
      return rc;
  }
  const uint64_t want_blocks = (n + 255) / 256;
  const uint32_t grid = (uint32_t)(want_blocks < (uint64_t)p->cu_count * 32 ? want_blocks : (uint64_t)p->cu_count * 32);
  std::vector<uint32_t> fresh;
  /* every pass but the last classifies a full list: at most KNOWN_MAX / CAP_MIN passes with a list
   * that never grows, far fewer with one that doubles */
  for (uint32_t round = 0; round < ACMPlan::CLS32_KNOWN_MAX / ACMPlan::CLS32_CAP_MIN + 64; round++) {
    HIP_TRY (hipMemsetAsync (p->d_unknown, 0, 4, st));
    HIP_TRY (launch (classify32_kernel, dim3 (grid), dim3 (256), 0, st, static_cast<const uint32_t *> (d_text),
                     static_cast<uint32_t *> (p->scratch.d_remap), n, p->d_cls32, p->cls32_slots - 1, p->d_unknown + 1, p->d_unknown,
                     p->cls32_cap));
    uint32_t cnt = 0;
    HIP_TRY (hipMemcpyWithStream (&cnt, p->d_unknown, 4, hipMemcpyDeviceToHost, st));
    if (cnt == 0)
      return ACM_GPU_OK;
    if (!p->cmp32)
      return ACM_GPU_E_INELIGIBLE; /* tables without their machine: nothing to classify new symbols with */
    const uint32_t listed = cnt < p->cls32_cap ? cnt : p->cls32_cap;
    if (p->cls32_known.size () + listed > ACMPlan::CLS32_KNOWN_MAX) {
      fprintf (stderr, "acm_gpu: the text brings more than %u distinct symbols to a comparator-class plan\n", ACMPlan::CLS32_KNOWN_MAX);
      return ACM_GPU_E_INELIGIBLE;
    }
    fresh.resize (listed);
    HIP_TRY (hipMemcpyWithStream (fresh.data (), p->d_unknown + 1, (size_t)listed * 4, hipMemcpyDeviceToHost, st));
    for (uint32_t sym : fresh)
      if (!p->cls32_known.count (sym))
        p->cls32_known[sym] = classify_symbol32 (p, sym);
    if (cnt >= p->cls32_cap && p->cls32_cap < ACMPlan::CLS32_CAP_MAX) {
      /* the list was full: the text has more to bring -- a longer list for the next pass */
      HIP_TRY (hipStreamSynchronize (st));
      HIP_TRY (hipFree (p->d_unknown));
      p->d_unknown = nullptr;
      p->cls32_cap *= 2;
      if (hipMalloc (reinterpret_cast<void **> (&p->d_unknown), (size_t)(p->cls32_cap + 1) * 4) != hipSuccess)
        return ACM_GPU_E_NOMEM;
    }
    rc = upload_cls32_table (p, st); /* also clears the slots claimed for symbols that did not fit the list */
    if (rc)
      return rc;
  }
  return ACM_GPU_E_INTERNAL;
}

/* The text the kernels walk: the caller's, or the plan's own copy of it in scratch.d_remap (*text is
 * redirected): interned ids, class ids, an aligned copy. */
int
prepare_text (ACMPlan *p, const void **text, uint64_t n, hipStream_t st) {
  const void *d_text = *text;
  const uint32_t sb = p->finfo.sym_bytes;
  if (p->d_intern) {
    /* 8-byte symbols: the kernels walk the 4-byte ids of the text */
    if (reinterpret_cast<uintptr_t> (d_text) & 7)
      return ACM_GPU_E_ARG;
    int rc = ensure_remap_buffer (p, (size_t)n * 4, st);
    if (rc)
      return rc;
    const uint64_t want_blocks = (n + 255) / 256;
    const uint32_t grid = (uint32_t)(want_blocks < (uint64_t)p->cu_count * 32 ? want_blocks : (uint64_t)p->cu_count * 32);
    HIP_TRY (launch (intern_kernel, dim3 (grid), dim3 (256), 0, st, static_cast<const uint64_t *> (d_text),
                     static_cast<uint32_t *> (p->scratch.d_remap), n, p->d_intern, p->intern_mask));
    *text = p->scratch.d_remap;
  } else if (p->cls32) {
    int rc = classify_text32 (p, d_text, n, st);
    if (rc)
      return rc;
    *text = p->scratch.d_remap;
  } else if (p->d_classlut) {
    /* comparator-class plan: walk the class ids of the text (our own, aligned, copy) */
    int rc = classmap_text (p, d_text, n, st);
    if (rc)
      return rc;
    *text = p->scratch.d_remap;
  } else if ((p->kind == PlanKind::Starts || p->kind == PlanKind::Gram) && (reinterpret_cast<uintptr_t> (d_text) & 15) != 0) {
    /* start-parallel / 4-gram plan, buffer not 16-byte aligned: scan an aligned copy (the CSR walk that
     * would take it as it is runs 20x slower, and knows nothing of incremental updates) */
    int rc = ensure_remap_buffer (p, (size_t)n * sb, st);
    if (rc)
      return rc;
    HIP_TRY (hipMemcpyAsync (p->scratch.d_remap, d_text, (size_t)n * sb, hipMemcpyDeviceToDevice, st));
    *text = p->scratch.d_remap;
  }
  return ACM_GPU_OK;
}

/* every segment of a scan restarts from the root `halo` symbols early: the longest keyword less
 * one, rounded up to a multiple of 16 bytes so that the kernels keep their alignment */
uint64_t
scan_halo (uint32_t lmax) {
  return lmax > 1 ? (((uint64_t)lmax - 1 + 15) / 16) * 16 : 0;
}

/* One launch's share of a scan of n symbols that reports from emit_from on: the symbols
 * [read_begin, read_begin + n) of the text, matches that end at emit_from (relative to read_begin)
 * or later.  Segments are at most ACMPlan::segment symbols plus the halo in front. */
struct Segment {
  uint64_t read_begin;
  uint32_t n, emit_from;
  bool first, last;
};

/* f (const Segment &) for every segment of the scan, until one fails */
template <typename F>
int
for_each_segment (const ACMPlan *p, uint64_t n, uint64_t emit_from, uint64_t halo, F f) {
  const uint64_t SEG = p->segment;
  const uint64_t first_seg = emit_from / SEG * SEG; /* earlier segments have nothing to report */
  for (uint64_t seg = first_seg; seg < n; seg += SEG) {
    const uint64_t seg_end = seg + SEG < n ? seg + SEG : n;
    const uint64_t read_begin = seg > halo ? seg - halo : 0;
    const uint64_t ef = emit_from > seg ? emit_from : seg;
    const Segment S = { read_begin, (uint32_t)(seg_end - read_begin), (uint32_t)(ef - read_begin), seg == first_seg, seg_end == n };
    const int rc = f (S);
    if (rc)
      return rc;
  }
  return ACM_GPU_OK;
}

/* what the launches of one scan have in common; the segment (text, n, emit_from, pos_base) is set
 * per launch.  spill: records past `capacity` go to the plan's spill area (scans whose kernel writes
 * the records itself); chunk_prev: the chunk links of a tiled scan. */
EmitCtx
make_emit_ctx (const ACMPlan *p, ACMRecord *records, uint64_t capacity, unsigned long long *count, uint32_t rec_chunk, bool spill,
               uint32_t *chunk_prev) {
  EmitCtx E{};
  E.oinfo = p->d_oinfo;
  E.records = records;
  E.count = count;
  E.capacity = capacity;
  E.wrows = p->d_wrows;
  E.cont_dh = p->d_cont_dh;
  E.W = p->K.W;
  E.lo = p->K.lo;
  E.span = p->K.span;
  E.chunk = p->chunk;
  E.n_states = p->finfo.n_states;
  E.kw4 = p->d_kw4;
  E.chain = p->d_chain;
  E.chain_base = p->K.HD;
  E.spill = static_cast<uint4 *> (p->scratch.d_spill);
  E.spill_slots = spill ? (uint64_t)p->scratch.direct_regions * rec_chunk : 0;
  E.rec_chunk = rec_chunk;
  E.chunk_prev = chunk_prev;
  E.error = error_word (p);
  return E;
}

/* tiled_scan: the scan is one of scan_tiled's (a Gram plan over a narrow alphabet, with records) */
template <bool COUNT_ONLY>
int
scan_impl (ACMPlan *p, const void *d_text, uint64_t n, uint64_t emit_from, uint64_t pos_base, ACMRecord *d_records,
           uint64_t capacity, uint64_t *d_count, hipStream_t st, bool accumulate = false, unsigned long long *shared_total = nullptr,
           TiledScan *tiled_scan = nullptr) {
  /* shared_total (with accumulate): the running total of ANOTHER plan to add to -- a delta plan
   * appends its records to those of the plan it belongs to */
  /* accumulate (streaming): records are appended after those of earlier calls -- the plan's
   * running total keeps counting and is handed over by acm_gpu_stream_finish, not here */
  HIP_TRY (hipSetDevice (p->device));
  const uint32_t sb = p->finfo.sym_bytes;
  /* (a comparator-class plan walks its own aligned copy of the text) */
  const bool use_dense = p->kind == PlanKind::Dense && (p->d_classlut || (reinterpret_cast<uintptr_t> (d_text) & 15) == 0);
  if (!accumulate && (n == 0 || p->finfo.n_edges == 0 || emit_from >= n || !use_dense))
    HIP_TRY (hipMemsetAsync (d_count, 0, sizeof (uint64_t), st));
  if (n == 0 || p->finfo.n_edges == 0 || emit_from >= n)
    return ACM_GPU_OK;
  if (p->mir && (p->mir->full_upload || !p->mir->patches.empty ())) {
    int rc = starts_flush (p, st); /* dictionary updates since the last scan */
    if (rc)
      return rc;
  }
  int rc = prepare_text (p, &d_text, n, st);
  if (rc)
    return rc;

  /* what kind of scan this is */
  const bool gram = p->kind == PlanKind::Gram;
  const bool direct = gram && !p->hashed; /* records straight from the scan kernel: no item buffer */
  const bool tiled = !COUNT_ONLY && direct && tiled_scan != nullptr;
  /* slots per chunk of records (EmitCtx::rec_chunk): big chunks for long texts, when no directory
   * of tiles counts in chunks (ACM_GPU_REC_CHUNK=1024 / 4096: one or the other anyway -- tests) */
  uint32_t rec_chunk = (!tiled && n >= (64ull << 20)) ? REC_CHUNK_BIG : REC_CHUNK;
  if (const char *e = getenv ("ACM_GPU_REC_CHUNK"))
    if (!tiled && (atoi (e) == (int)REC_CHUNK || atoi (e) == (int)REC_CHUNK_BIG))
      rec_chunk = (uint32_t)atoi (e);

  if (use_dense || (!COUNT_ONLY && !direct && (gram || p->kind == PlanKind::Starts))) {
    /* 4-gram plans over hashed windows see dense matches: room for one hit per 16 symbols, per 8
     * when the dictionary has keywords of 1-3 symbols; past that a wave reserves records 64 at a time */
    rc = ensure_item_buffer (p, n < p->segment ? n : p->segment, gram ? (p->inline_shorts ? 8 : 16) : 256,
                             use_dense ? DENSE_MIN_REGION_ITEMS : 256);
    if (rc)
      return rc;
  }
  if (!COUNT_ONLY && direct) {
    rc = ensure_direct_buffers (p, rec_chunk);
    if (rc)
      return rc;
  }

  unsigned long long *const count =
    shared_total ? shared_total : ((use_dense || accumulate || tiled) ? p->scratch.d_total : reinterpret_cast<unsigned long long *> (d_count));
  EmitCtx E = make_emit_ctx (p, d_records, COUNT_ONLY ? 0 : capacity, count, rec_chunk, !COUNT_ONLY && direct && !tiled,
                             tiled ? tiled_scan->chunk_prev : nullptr);
  uint32_t holes_waves[2] = { 0, 0 }; /* widest launch so far of the 4-gram pass, of the short-keyword pass */

  /* one pass over the segments of the text; `launch` makes the launches of one */
  auto pass = [&] (uint64_t halo, auto launch) -> int {
    return for_each_segment (p, n, emit_from, halo, [&] (const Segment &S) -> int {
      Launch a{};
      a.text = static_cast<const unsigned char *> (d_text) + S.read_begin * sb;
      a.n = S.n;
      a.emit_from = S.emit_from;
      E.pos_base = pos_base + S.read_begin;
      E.text = a.text;
      E.n = a.n;
      E.emit_from = a.emit_from;
      hipEvent_t stop, stop_all;
      int rc = timing_begin (p, st, &stop, &stop_all);
      if (rc)
        return rc;
      rc = launch (a, stop, S.first, S.last);
      if (!rc && stop_all) /* behind the expansion / hole closing the launch functions enqueue after their scan kernel */
        HIP_TRY (hipEventRecord (stop_all, st));
      return rc;
    });
  };
  auto main_pass = [&] (Launch &a, hipEvent_t stop, bool first_segment, bool last_segment) -> int {
    int rc = ACM_GPU_OK;
    const bool aligned = (reinterpret_cast<uintptr_t> (a.text) & 15) == 0;
    if (use_dense)
      rc = launch_dense<COUNT_ONLY> (p, E, a, st, stop, d_count, last_segment && !accumulate);
    else {
      a.range_begin = 0;
      a.range_end = a.n;
      if (gram)
        rc = launch_gram<COUNT_ONLY> (p, E, a, st, stop, first_segment, last_segment, holes_waves[0], tiled ? tiled_scan : nullptr);
      else if (p->kind == PlanKind::Starts && aligned)
        rc = launch_starts<COUNT_ONLY> (p, E, a, st, stop);
      else {
        /* (the CSR walk takes any alignment: a Dense plan's unaligned text, a Starts plan's unaligned segment) */
        if ((p->kind == PlanKind::Sparse || p->kind == PlanKind::Starts) && aligned)
          rc = launch_sparse<COUNT_ONLY> (p, E, a, st);
        else
          rc = launch_csr<COUNT_ONLY> (p, E, a, st);
        if (!rc && stop)
          HIP_TRY (hipEventRecord (stop, st));
      }
    }
    /* earlier segments may have left a partial running total and expand ticket behind */
    if (rc && use_dense && p->scratch.d_total)
      (void)hipMemsetAsync (p->scratch.d_total, 0, 16, st);
    return rc;
  };
  rc = pass (scan_halo (p->finfo.lmax), main_pass);
  /* narrow alphabets: the keywords of 1-3 symbols, a pass of their own over the same segments
   * (dev_short.h); their records follow the 4-gram pass' in the same buffer.  (A halo of 2 symbols
   * would do: 16 keeps the alignment.) */
  if (!rc && gram && p->short_pass)
    rc = pass (16, [&] (Launch &a, hipEvent_t stop, bool first_segment, bool last_segment) {
      return launch_short<COUNT_ONLY> (p, E, a, st, stop, first_segment, last_segment, holes_waves[1]);
    });
  return rc;
}

/* deltas replaced since the last call that used the plan's delta: whatever may still use them is on
 * this stream, in front of this mark */
int
mark_retired (ACMPlan *p, hipStream_t st) {
  if (p->retired.empty ())
    return ACM_GPU_OK;
  HIP_TRY (hipSetDevice (p->device));
  for (auto &r : p->retired)
    if (!r.done) {
      HIP_TRY (hipEventCreateWithFlags (&r.done, hipEventDisableTiming));
      HIP_TRY (hipEventRecord (r.done, st));
    }
  return ACM_GPU_OK;
}

/* a plan and, if it has one, its delta (acm_gpu_plan_update): both scans append to the same record
 * buffer through the plan's running total, handed to the caller's counter at the end */
template <bool COUNT_ONLY>
int
scan_plan (ACMPlan *p, const void *d_text, uint64_t n, uint64_t emit_from, uint64_t pos_base, ACMRecord *d_records,
           uint64_t capacity, uint64_t *d_count, hipStream_t st, bool accumulate = false) {
  if (const int rc = mark_retired (p, st))
    return rc;
  if (!p->delta)
    return scan_impl<COUNT_ONLY> (p, d_text, n, emit_from, pos_base, d_records, capacity, d_count, st, accumulate);
  int rc = scan_impl<COUNT_ONLY> (p, d_text, n, emit_from, pos_base, d_records, capacity, d_count, st, true);
  if (!rc)
    rc = scan_impl<COUNT_ONLY> (p->delta, d_text, n, emit_from, pos_base, d_records, capacity, d_count, st, true, p->scratch.d_total);
  p->delta_scanned += n; /* what acm_gpu_plan_update weighs against the cost of one plan of everything */
  if (!accumulate) { /* (also after a failure: the total must not leak into the next scan) */
    HIP_TRY (launch (finish_count_kernel, dim3 (1), dim3 (64), 0, st, p->scratch.d_total, reinterpret_cast<unsigned long long *> (d_count)));
  }
  return rc;
}

} // namespace

extern "C" int
acm_gpu_scan_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from, uint64_t pos_base,
                     ACMRecord *d_records, uint64_t capacity, uint64_t *d_count, void *stream) {
  if (!plan || !d_count || (n_symbols && !d_text) || (capacity && !d_records))
    return ACM_GPU_E_ARG;
  return scan_plan<false> (plan, d_text, n_symbols, emit_from, pos_base, d_records, capacity, d_count,
                           static_cast<hipStream_t> (stream));
}

extern "C" int
acm_gpu_count_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from, uint64_t *d_count,
                      void *stream) {
  if (!plan || !d_count || (n_symbols && !d_text))
    return ACM_GPU_E_ARG;
  return scan_plan<true> (plan, d_text, n_symbols, emit_from, 0, nullptr, 0, d_count, static_cast<hipStream_t> (stream));
}

/* ------------------------------------------------------------------ streaming scan
 * The reference's callers read their text piece by piece (generic_test.c:191 uses fgetwc) and the
 * scan is resumable by construction: the cursor depends on the last lmax symbols only.  A stream
 * keeps two device slots; piece k is copied into slot k % 2 on a copy stream while piece k - 1 is
 * scanned on the compute stream; the last `halo` symbols of the stream so far are placed in front
 * of every piece so that matches straddling pieces are found (reported once: emit_from = halo). */
struct ACMStream {
  ACMPlan *plan = nullptr;
  uint32_t sb = 1;
  uint64_t halo = 0, max_piece = 0;
  unsigned char *slot[2] = { nullptr, nullptr }; /* (halo + max_piece) symbols each */
  hipStream_t copy = nullptr, compute = nullptr;
  hipEvent_t copied[2] = { nullptr, nullptr }, scanned[2] = { nullptr, nullptr }, tail_read[2] = { nullptr, nullptr };
  ACMRecord *d_records = nullptr;
  uint64_t capacity = 0;
  uint64_t position = 0; /* symbols fed so far */
  uint64_t pieces = 0;
  uint64_t prev_valid = 0; /* context + piece symbols held, contiguously, by the previous slot */
  uint64_t last_piece = 0; /* length of the previous piece */
};

extern "C" int
acm_gpu_stream_open (ACMPlan *plan, uint64_t max_piece_symbols, uint64_t record_capacity, ACMStream **out) {
  if (!plan || !out || max_piece_symbols == 0)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  ACMStream *s = new (std::nothrow) ACMStream ();
  if (!s)
    return ACM_GPU_E_NOMEM;
  s->plan = plan;
  s->sb = plan->text_sym_bytes; /* of the caller's text (8-byte symbols are interned inside the scan) */
  s->halo = scan_halo (plan->finfo.lmax);
  s->max_piece = (max_piece_symbols + 15) / 16 * 16;
  s->capacity = record_capacity;
  const size_t slot_bytes = (size_t)(s->halo + s->max_piece) * s->sb + 16;
  bool ok = hipMalloc (reinterpret_cast<void **> (&s->slot[0]), slot_bytes) == hipSuccess &&
            hipMalloc (reinterpret_cast<void **> (&s->slot[1]), slot_bytes) == hipSuccess &&
            hipMalloc (reinterpret_cast<void **> (&s->d_records), (record_capacity ? record_capacity : 1) * sizeof (ACMRecord)) == hipSuccess &&
            hipStreamCreateWithFlags (&s->copy, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags (&s->compute, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; ok && i < 2; i++)
    ok = hipEventCreateWithFlags (&s->copied[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags (&s->scanned[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags (&s->tail_read[i], hipEventDisableTiming) == hipSuccess;
  /* a stream owns the plan's running total while it is open: start from zero.  Earlier scans of
   * the plan (on whatever stream) must have drained, and the memset (null stream) must have landed
   * before the stream's own non-blocking streams touch the total: without the waits a warm
   * process lost the first piece's count now and then */
  ok = ok && hipDeviceSynchronize () == hipSuccess && hipMemset (plan->scratch.d_total, 0, 8) == hipSuccess &&
       hipDeviceSynchronize () == hipSuccess;
  if (!ok) {
    acm_gpu_stream_close (s);
    return ACM_GPU_E_NOMEM;
  }
  *out = s;
  return ACM_GPU_OK;
}

/* Feeds the next n_symbols of the stream from HOST memory (pinned memory makes the copy truly
 * asynchronous).  Returns as soon as the copy and the scan are enqueued; `text` must stay
 * untouched until the second next feed or acm_gpu_stream_finish has returned: before a slot is
 * filled again the host waits for the copy that filled it two pieces ago, so by the time feed k
 * returns the buffers of the pieces up to k - 2 have been read. */
extern "C" int
acm_gpu_stream_feed (ACMStream *s, const void *text, uint64_t n_symbols) {
  if (!s || (n_symbols && !text))
    return ACM_GPU_E_ARG;
  ACMPlan *p = s->plan;
  HIP_TRY (hipSetDevice (p->device));
  const unsigned char *src = static_cast<const unsigned char *> (text);
  while (n_symbols) {
    const uint64_t n = n_symbols < s->max_piece ? n_symbols : s->max_piece;
    const int cur = (int)(s->pieces & 1), prev = cur ^ 1;
    unsigned char *piece_at = s->slot[cur] + s->halo * s->sb;
    /* the slot is free once the scan that used it two pieces ago is done and the previous piece
     * has taken its context from the slot's tail */
    if (s->pieces >= 2) {
      HIP_TRY (hipEventSynchronize (s->copied[cur])); /* the caller may now reuse that piece's buffer */
      HIP_TRY (hipStreamWaitEvent (s->copy, s->scanned[cur], 0));
    }
    if (s->pieces >= 1)
      HIP_TRY (hipStreamWaitEvent (s->copy, s->tail_read[cur], 0));
    HIP_TRY (hipMemcpyAsync (piece_at, src, (size_t)n * s->sb, hipMemcpyHostToDevice, s->copy));
    HIP_TRY (hipEventRecord (s->copied[cur], s->copy));
    /* context: the last `ctx` symbols the previous slot holds, end-aligned in front of the piece */
    const uint64_t ctx = s->prev_valid < s->halo ? s->prev_valid : s->halo;
    HIP_TRY (hipStreamWaitEvent (s->compute, s->copied[cur], 0));
    if (ctx) {
      const unsigned char *tail = s->slot[prev] + (s->halo + s->last_piece - ctx) * s->sb;
      HIP_TRY (hipMemcpyAsync (piece_at - ctx * s->sb, tail, (size_t)ctx * s->sb, hipMemcpyDeviceToDevice, s->compute));
    }
    HIP_TRY (hipEventRecord (s->tail_read[prev], s->compute));
    int rc = scan_plan<false> (p, piece_at - ctx * s->sb, ctx + n, ctx, s->position - ctx, s->d_records, s->capacity, nullptr,
                               s->compute, true);
    if (rc)
      return rc;
    HIP_TRY (hipEventRecord (s->scanned[cur], s->compute));
    s->prev_valid = ctx + n;
    s->last_piece = n;
    s->position += n;
    s->pieces++;
    src += (size_t)n * s->sb;
    n_symbols -= n;
  }
  return ACM_GPU_OK;
}

/* Waits for everything fed so far, puts the records in canonical order and copies them to the
 * host.  *n_found = matches of the whole stream so far (ACM_GPU_E_OVERFLOW if more than the
 * stream's record capacity or than `capacity`).  The stream stays open and keeps accumulating. */
extern "C" int
acm_gpu_stream_finish (ACMStream *s, ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  if (!s || !n_found)
    return ACM_GPU_E_ARG;
  ACMPlan *p = s->plan;
  HIP_TRY (hipSetDevice (p->device));
  HIP_TRY (hipStreamSynchronize (s->copy));
  HIP_TRY (hipStreamSynchronize (s->compute));
  unsigned long long total = 0;
  HIP_TRY (hipMemcpy (&total, p->scratch.d_total, 8, hipMemcpyDeviceToHost));
  *n_found = total;
  if (total > s->capacity || total > capacity)
    return ACM_GPU_E_OVERFLOW;
  if (total > 1) {
    const size_t tb = acm_gpu_order_tmp_bytes (p, total, s->position);
    DeviceTemps temps;
    void *tmp = nullptr;
    if (temps.get (&tmp, tb) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    int rc = acm_gpu_order_records_device (p, s->d_records, total, 0, s->position, tmp, tb, s->compute);
    if (!rc && hipStreamSynchronize (s->compute) != hipSuccess)
      rc = ACM_GPU_E_HIP;
    if (rc)
      return rc;
  }
  if (total && records)
    HIP_TRY (hipMemcpy (records, s->d_records, total * sizeof (ACMRecord), hipMemcpyDeviceToHost));
  return acm_gpu_plan_status (p);
}

extern "C" void
acm_gpu_stream_close (ACMStream *s) {
  if (!s)
    return;
  (void)hipSetDevice (s->plan->device);
  if (s->copy)
    (void)hipStreamSynchronize (s->copy);
  if (s->compute)
    (void)hipStreamSynchronize (s->compute);
  (void)hipMemset (s->plan->scratch.d_total, 0, 8); /* hand the plan back with a clean running total */
  (void)hipDeviceSynchronize ();
  for (int i = 0; i < 2; i++) {
    if (s->slot[i]) (void)hipFree (s->slot[i]);
    if (s->copied[i]) (void)hipEventDestroy (s->copied[i]);
    if (s->scanned[i]) (void)hipEventDestroy (s->scanned[i]);
    if (s->tail_read[i]) (void)hipEventDestroy (s->tail_read[i]);
  }
  if (s->d_records) (void)hipFree (s->d_records);
  if (s->copy) (void)hipStreamDestroy (s->copy);
  if (s->compute) (void)hipStreamDestroy (s->compute);
  delete s;
}

/* ------------------------------------------------------------------ canonical order */
namespace {
size_t
cub_sort_bytes (uint64_t n) {
  size_t tmp = 0;
  hipcub::DoubleBuffer<uint64_t> k (nullptr, nullptr);
  hipcub::DoubleBuffer<Rec16> v (nullptr, nullptr);
  (void)hipcub::DeviceRadixSort::SortPairs (nullptr, tmp, k, v, (int)n, 0, 64, nullptr);
  return tmp;
}
size_t
align256 (size_t x) {
  return (x + 255) & ~(size_t)255;
}
} // namespace

extern "C" size_t
acm_gpu_sort_tmp_bytes (uint64_t n) {
  if (n == 0)
    return 256;
  return align256 (n * 8) * 2 + align256 (n * 16) + align256 (cub_sort_bytes (n)) + 256;
}

namespace {
int radix_sort_records (ACMPlan *plan, ACMRecord *d_records, uint64_t n, void *d_tmp, size_t tmp_bytes, void *stream, uint64_t pos_lo, int pos_bits);
}

extern "C" int
acm_gpu_sort_records_device (ACMPlan *plan, ACMRecord *d_records, uint64_t n, void *d_tmp, size_t tmp_bytes, void *stream) {
  return radix_sort_records (plan, d_records, n, d_tmp, tmp_bytes, stream, 0, 64);
}

namespace {
/* Two stable radix sorts: by ~length (all 32 bits), then by end_pos - pos_lo (its low pos_bits bits:
 * a caller that knows the range of the positions saves the radix passes over bits that are zero).
 * The second keeps the first's order among equal positions, so the result is the canonical order
 * for ANY 64-bit end_pos and ANY 32-bit length -- one key of (position << len_bits | max - length)
 * loses the top len_bits bits of the position and every length above the plan's lmax.  Both sorts
 * use the same key and value buffers, so the scratch is that of one. */
int
radix_sort_records (ACMPlan *plan, ACMRecord *d_records, uint64_t n, void *d_tmp, size_t tmp_bytes, void *stream, uint64_t pos_lo, int pos_bits) {
  if (!plan || (n && (!d_records || !d_tmp)))
    return ACM_GPU_E_ARG;
  if (n <= 1)
    return ACM_GPU_OK;
  if (n >= (1ull << 31) || tmp_bytes < acm_gpu_sort_tmp_bytes (n))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  unsigned char *t = static_cast<unsigned char *> (d_tmp);
  uint64_t *k0 = reinterpret_cast<uint64_t *> (t);
  uint64_t *k1 = reinterpret_cast<uint64_t *> (t + align256 (n * 8));
  Rec16 *v0 = reinterpret_cast<Rec16 *> (d_records);
  Rec16 *v1 = reinterpret_cast<Rec16 *> (t + 2 * align256 (n * 8));
  void *cub_tmp = t + 2 * align256 (n * 8) + align256 (n * 16);
  size_t cub_bytes = cub_sort_bytes (n);
  const dim3 kgrid ((uint32_t)((n + 255) / 256));
  HIP_TRY (launch (make_keys_kernel<false>, kgrid, dim3 (256), 0, st, d_records, n, (uint64_t)0, k0));
  hipcub::DoubleBuffer<uint64_t> lkeys (k0, k1);
  hipcub::DoubleBuffer<Rec16> lvals (v0, v1);
  HIP_TRY (hipcub::DeviceRadixSort::SortPairs (cub_tmp, cub_bytes, lkeys, lvals, (int)n, 0, 32, st));
  Rec16 *by_len = lvals.Current (), *other = by_len == v0 ? v1 : v0;
  HIP_TRY (launch (make_keys_kernel<true>, kgrid, dim3 (256), 0, st, reinterpret_cast<const ACMRecord *> (by_len), n, pos_lo, k0));
  hipcub::DoubleBuffer<uint64_t> pkeys (k0, k1);
  hipcub::DoubleBuffer<Rec16> pvals (by_len, other);
  HIP_TRY (hipcub::DeviceRadixSort::SortPairs (cub_tmp, cub_bytes, pkeys, pvals, (int)n, 0, pos_bits, st));
  if (pvals.Current () != v0)
    HIP_TRY (hipMemcpyAsync (d_records, pvals.Current (), n * 16, hipMemcpyDeviceToDevice, st));
  return ACM_GPU_OK;
}
} // namespace

/* ---- canonical order of records whose positions lie in [pos_lo, pos_lo + span): dev_order.h */
namespace {
struct OrderPlan {
  uint32_t wlog = 0, n_buckets = 0, len_bits = 1, pos_bits = 64; /* pos_bits: the smallest b with 2^b >= span */
  bool sparse = false; /* fewer than 8 records per 4,096 positions: pass C goes by windows of buckets, not by bucket */
  uint32_t *hist = nullptr, *cur = nullptr; /* the scratch, bound when the carve has a base */
  ACMRecord *bucketed = nullptr;
  CubRoom cub;
  size_t total = 0;
  bool ok = false;
};
OrderPlan
order_layout (const ACMPlan *plan, uint64_t n, uint64_t span, Carve c = Carve ()) {
  OrderPlan L;
  if (n == 0 || span == 0 || n >= (1ull << 31))
    return L;
  uint32_t span_bits = 1;
  while ((1ull << span_bits) < span && span_bits < 63)
    span_bits++;
  const uint32_t len_bits = len_bits_of (plan_lmax (plan));
  L.len_bits = len_bits;
  L.pos_bits = (1ull << span_bits) < span ? 64 : span_bits;
  /* buckets of ORDER_POSITIONS positions (fewer when the whole range is shorter): whatever a
   * bucket holds, order_count_role has a counter per position for it */
  uint32_t wlog = 0;
  while ((2u << wlog) <= ORDER_POSITIONS && (1ull << wlog) < span)
    wlog++;
  L.sparse = order_is_sparse (n, span);
  const uint64_t nb = (span >> wlog) + 1;
  if (nb >= (1ull << 28) || span_bits + len_bits > 63 || wlog + len_bits > 31) /* (a bucket's keys are 32-bit) */
    return L;
  L.wlog = wlog;
  L.n_buckets = (uint32_t)nb;
  L.hist = c.take<uint32_t> ((nb + 1) + (nb + 2)); /* counts, then (cur, right behind them) a zero word and the sums */
  L.cur = L.hist ? L.hist + (nb + 1) : nullptr;
  L.bucketed = c.take<ACMRecord> (n);
  L.cub = cub_room (c, nb + 1, 0);
  L.total = c.total ();
  L.ok = true;
  return L;
}
} // namespace

extern "C" size_t
acm_gpu_order_tmp_bytes (const ACMPlan *plan, uint64_t n, uint64_t span) {
  if (!plan)
    return 0;
  const OrderPlan L = order_layout (plan, n, span);
  const size_t radix = acm_gpu_sort_tmp_bytes (n);
  return L.ok && L.total > radix ? L.total : radix; /* (room for the fallback either way) */
}

namespace {
/* what is cleared in front of pass A: the counts and cur[0] -- rounded up to whole 256 bytes (one
 * fill kernel instead of a body and a tail; what lies behind is the sums' own space) */
size_t
order_zero_bytes (const OrderPlan &L) {
  return (((size_t)L.n_buckets + 2) * 4 + 255) & ~(size_t)255;
}

/* n_dev == nullptr: n records.  Else: the record count is the scan's, in device memory, and n the
 * capacity of d_records (OrderK::n_dev) -- nothing here waits for the host. */
bool
order_by_buckets (const ACMPlan *plan, const OrderPlan &L) {
  const char *env = getenv ("ACM_GPU_ORDER"); /* radix: always the radix sort (experiments, tests) */
  (void)plan;
  return L.ok && !(env && strcmp (env, "radix") == 0);
}

int
order_records (ACMPlan *plan, ACMRecord *d_records, uint64_t n, const unsigned long long *n_dev, uint64_t pos_lo, uint64_t span, void *d_tmp,
               size_t tmp_bytes, void *stream) {
  if (tmp_bytes < acm_gpu_order_tmp_bytes (plan, n, span))
    return ACM_GPU_E_ARG;
  const OrderPlan L = order_layout (plan, n, span, Carve (d_tmp));
  if (!order_by_buckets (plan, L)) {
    if (n_dev)
      return ACM_GPU_E_ARG; /* (the caller asks order_by_buckets first) */
    return radix_sort_records (plan, d_records, n, d_tmp, tmp_bytes, stream, pos_lo, (int)L.pos_bits);
  }
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  uint32_t *hist = L.hist, *cur = L.cur;
  ACMRecord *bucketed = L.bucketed;
  OrderK K{};
  K.in = d_records;
  K.n = n;
  K.pos_lo = pos_lo;
  K.wlog = L.wlog;
  K.n_buckets = L.n_buckets;
  K.len_bits = L.len_bits;
  K.error = error_word (plan);
  K.n_dev = n_dev;
  K.span = span;
  K.mode = n_dev ? 2u : (L.sparse ? 1u : 0u);
  /* `hist`: the buckets' counts (pass A).  `cur`: one word that stays 0, then the buckets' exclusive
   * prefix sums -- where each bucket begins, the cursors pass B advances; when it is done cur[1 + b]
   * is where bucket b ENDS, so that P = cur reads P[b] = begin, P[b + 1] = end for pass C (no copy
   * of the sums is kept) */
  const uint64_t pieces = (n + ORDER_PIECE - 1) / ORDER_PIECE, pblocks = (pieces + ORDER_THREADS / WAVE - 1) / (ORDER_THREADS / WAVE);
  const dim3 grid = capped_grid (plan, pblocks);
  HIP_TRY (hipMemsetAsync (hist, 0, order_zero_bytes (L), st)); /* (the counts and cur[0], which lies right behind them) */
  HIP_TRY (launch (order_bucket_kernel<false>, grid, dim3 (ORDER_THREADS), 0, st, K, hist, static_cast<ACMRecord *> (nullptr)));
  HIP_TRY (exclusive_sum (L.cub, hist, cur + 1, L.n_buckets + 1, st));
  HIP_TRY (launch (order_bucket_kernel<true>, grid, dim3 (ORDER_THREADS), 0, st, K, cur + 1, bucketed));
  /* pass C: buckets (dense record sets) or windows of buckets (sparse ones) of up to 256 records by
   * a wave each, crowded buckets by a block each (each role skips the others' buckets); a role
   * that does not run keeps a grid of zero */
  uint32_t wgrid = 0, sgrid = 0;
  if (n_dev || L.sparse) { /* (with the count on the device both are there: the one whose kind of set it is not returns at once) */
    const uint64_t windows = (n + ORDER_WINDOW - 1) / ORDER_WINDOW, wblocks = (windows + 3) / 4;
    wgrid = capped_grid (plan, wblocks, 16).x;
  }
  if (n_dev || !L.sparse)
    sgrid = capped_grid (plan, (L.n_buckets + 3) / 4, 16).x;
  const uint32_t cgrid = capped_grid (plan, (L.n_buckets + ORDER_COUNT_THREADS - 1) / ORDER_COUNT_THREADS).x;
  HIP_TRY (launch (order_finish_kernel, dim3 (wgrid + sgrid + cgrid), dim3 (256), 0, st, K, cur, bucketed, d_records, wgrid, sgrid));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_order_records_device (ACMPlan *plan, ACMRecord *d_records, uint64_t n, uint64_t pos_lo, uint64_t span, void *d_tmp,
                              size_t tmp_bytes, void *stream) {
  if (!plan || (n && (!d_records || !d_tmp)))
    return ACM_GPU_E_ARG;
  if (n <= 1)
    return ACM_GPU_OK;
  return order_records (plan, d_records, n, nullptr, pos_lo, span, d_tmp, tmp_bytes, stream);
}

/* ---- tiled scans (dev_tiles.h): 4-gram plans over narrow alphabets */
namespace {
struct TiledPlan {
  bool ok = false;
  uint32_t n_tiles = 0;
  uint64_t raw_slots = 0;
  uint32_t len_bits = 1, nsub = 2;
  ACMRecord *raw = nullptr; /* the scratch, bound when the carve has a base */
  uint32_t *prev = nullptr, *size = nullptr, *begin = nullptr, *crowded = nullptr;
  TileEntry *dir = nullptr;
  unsigned long long *over = nullptr;
  CubRoom cub;
  size_t total = 0;
};

/* the tiles of all the launches scan_impl makes for this text.
 * bound: an upper bound of the layout over every emit_from (acm_gpu_scan_ordered_tmp_bytes): the
 * tiles are counted at the smallest R gram_tiling ever picks.  (Round 3 sized the scratch with
 * emit_from = 0 "for the most tiles" -- but R = clamp (groups behind emit_from / (16 per wave), 4,
 * 64), so a later emit_from can LOWER R and give more tiles than emit_from = 0: 1 GiB on 256 CUs
 * is 16,384 tiles at emit_from = 0 and 20,480 when 81,919 groups are left.) */
TiledPlan
tiled_layout (const ACMPlan *p, uint64_t capacity, uint64_t n, uint64_t emit_from, bool bound = false, Carve c = Carve ()) {
  TiledPlan L;
  const char *env = getenv ("ACM_GPU_ORDER"); /* radix / buckets: not this way (experiments, tests) */
  if (env && (strcmp (env, "radix") == 0 || strcmp (env, "buckets") == 0))
    return L;
  if (p->kind != PlanKind::Gram || p->hashed || p->short_pass || p->delta || plan_lmax (p) > WAVE * 16 || p->finfo.n_edges == 0)
    return L; /* (a second pass' records do not lie tile by tile: the general order passes) */
  if (n == 0 || emit_from >= n || capacity == 0 || capacity >= (1ull << 31))
    return L;
  uint64_t tiles = 0;
  (void)for_each_segment (p, n, emit_from, scan_halo (p->finfo.lmax), [&] (const Segment &S) {
    TileGeometry T = gram_tiling (p, S.n, S.emit_from);
    if (bound) { /* every group of the segment, GRAM_R_MIN groups per tile */
      const uint32_t ngroups = (uint32_t)(((uint64_t)S.n + WAVE * 16 - 1) / (WAVE * 16));
      T.begin = 0;
      T.end = (ngroups + GRAM_R_MIN - 1) / GRAM_R_MIN;
    }
    tiles += T.end - T.begin;
    if (T.R * (WAVE * 16) / (1u << TILE_BUCKET_LOG2) + 1 > L.nsub)
      L.nsub = T.R * (WAVE * 16) / (1u << TILE_BUCKET_LOG2) + 1;
    return ACM_GPU_OK;
  });
  if (tiles == 0 || tiles >= (1ull << 30))
    return L;
  L.n_tiles = (uint32_t)tiles;
  /* whole chunks: the records and what every wave may leave unused of its last chunk */
  L.raw_slots = (capacity + REC_CHUNK - 1) / REC_CHUNK * REC_CHUNK + ((uint64_t)p->cu_count * (SPARSE_THREADS / WAVE) + 1) * REC_CHUNK;
  L.len_bits = len_bits_of (plan_lmax (p));
  L.raw = c.take<ACMRecord> (L.raw_slots);
  L.prev = c.take<uint32_t> (L.raw_slots / REC_CHUNK);
  L.dir = c.take<TileEntry> (L.n_tiles);
  L.size = c.take<uint32_t> ((size_t)L.n_tiles + 1);
  L.begin = c.take<uint32_t> ((size_t)L.n_tiles + 1);
  L.crowded = c.take<uint32_t> ((size_t)L.n_tiles + 1);
  L.over = c.take<unsigned long long> (1);
  L.cub = cub_room (c, (uint64_t)L.n_tiles + 1, 0);
  L.total = c.total ();
  L.ok = true;
  return L;
}

int
scan_tiled (ACMPlan *plan, const TiledPlan &L, const void *d_text, uint64_t n_symbols, uint64_t emit_from, uint64_t pos_base, ACMRecord *d_records,
            uint64_t capacity, uint64_t *d_count, hipStream_t st) {
  HIP_TRY (hipSetDevice (plan->device));
  TiledScan tiled = { L.dir, L.prev, 0 };
  int rc = scan_impl<false> (plan, d_text, n_symbols, emit_from, pos_base, L.raw, L.raw_slots, d_count, st, false, nullptr, &tiled);
  if (rc || tiled.base != L.n_tiles) { /* (the directory was sized by tiled_layout, filled by launch_gram) */
    (void)hipMemsetAsync (plan->scratch.d_total, 0, 8, st); /* (the scan's running total must not leak into the next one) */
    return rc ? rc : ACM_GPU_E_INTERNAL;
  }
  TileK K{};
  K.raw = L.raw;
  K.chunk_prev = L.prev;
  K.dir = L.dir;
  K.n_tiles = L.n_tiles;
  K.size = L.size;
  K.begin = L.begin;
  K.out = d_records;
  K.capacity = capacity;
  K.d_count = reinterpret_cast<unsigned long long *> (d_count);
  K.reserved = plan->scratch.d_total;
  K.len_bits = L.len_bits;
  K.nsub = L.nsub;
  K.crowded = L.crowded;
  K.raw_slots = L.raw_slots;
  K.over_total = L.over;
  HIP_TRY (hipMemsetAsync (K.over_total, 0, 8, st));
  K.error = error_word (plan);
  HIP_TRY (launch (tile_size_kernel, capped_grid (plan, (L.n_tiles + 1 + 3) / 4, 16), dim3 (256), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.size, L.begin, L.n_tiles + 1, st));
  HIP_TRY (launch (tile_gather_kernel, capped_grid (plan, L.n_tiles, 16), dim3 (TILE_THREADS), tile_lds_bytes (L.nsub), st, K));
  /* the tiles it found crowded (dense matches; none on ordinary texts: the kernel returns at once) */
  HIP_TRY (launch (tile_crowded_kernel, capped_grid (plan, L.n_tiles, 4), dim3 (TILE_THREADS), tile_lds_bytes (L.nsub), st, K));
  return ACM_GPU_OK;
}
} // namespace

/* Scan and canonical order in one call, nothing but kernel launches on `stream`: the order passes
 * take the number of records from *d_count on the device.  A scan that overflows `capacity` leaves
 * the total in *d_count as acm_gpu_scan_device does and nothing in order (the caller repeats it with
 * room).  4-gram plans over narrow alphabets scan in tiles and order in one pass (dev_tiles.h).
 * Record sets the bucket passes do not take (2^31 records or more, positions past 2^63 /
 * lengths): the count comes to the host and acm_gpu_order_records_device's fallback runs. */
extern "C" size_t
acm_gpu_scan_ordered_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols) {
  if (!plan)
    return 0;
  const size_t general = acm_gpu_order_tmp_bytes (plan, capacity, n_symbols);
  const TiledPlan L = tiled_layout (plan, capacity, n_symbols, 0, true); /* (an upper bound over every emit_from) */
  return L.ok && L.total > general ? L.total : general;
}

extern "C" int
acm_gpu_scan_ordered_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from, uint64_t pos_base,
                             ACMRecord *d_records, uint64_t capacity, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || (n_symbols && !d_text) || (capacity && (!d_records || !d_tmp)))
    return ACM_GPU_E_ARG;
  if (capacity && tmp_bytes < acm_gpu_scan_ordered_tmp_bytes (plan, capacity, n_symbols))
    return ACM_GPU_E_ARG;
  const TiledPlan T = tiled_layout (plan, capacity, n_symbols, emit_from, false, Carve (d_tmp));
  /* (the layout of THIS emit_from must fit what the caller gave -- the query is an upper bound, so
   * it does; a buffer sized some other way takes the general passes, never a write past its end) */
  if (T.ok && T.total <= tmp_bytes)
    return scan_tiled (plan, T, d_text, n_symbols, emit_from, pos_base, d_records, capacity, d_count, static_cast<hipStream_t> (stream));
  const OrderPlan L = order_layout (plan, capacity, n_symbols);
  int rc = acm_gpu_scan_device (plan, d_text, n_symbols, emit_from, pos_base, d_records, capacity, d_count, stream);
  if (rc || capacity == 0 || n_symbols == 0)
    return rc;
  if (order_by_buckets (plan, L))
    return order_records (plan, d_records, capacity, reinterpret_cast<const unsigned long long *> (d_count), pos_base, n_symbols, d_tmp, tmp_bytes, stream);
  uint64_t found = 0;
  HIP_TRY (hipMemcpyAsync (&found, d_count, 8, hipMemcpyDeviceToHost, static_cast<hipStream_t> (stream)));
  HIP_TRY (hipStreamSynchronize (static_cast<hipStream_t> (stream)));
  if (found <= 1 || found > capacity)
    return ACM_GPU_OK;
  return order_records (plan, d_records, found, nullptr, pos_base, n_symbols, d_tmp, tmp_bytes, stream);
}

/* ------------------------------------------------------------------ host-buffer convenience */
namespace {
/* what a batch brings down beside its records */
struct BatchDownload {
  uint32_t *text_id;
  const uint32_t *d_text_id;
  uint64_t *first;
  const uint64_t *d_first;
  uint64_t n_texts;
  bool first_on_overflow = false; /* the call leaves d_first complete when the records had no room (anchored): first[] comes down then too */
};

/* the end of a host convenience, behind its device call (which gave rc): the count, *n_found,
 * ACM_GPU_E_OVERFLOW when the records had no room, else `order (found)` and the records (with a
 * batch's text ids and first[]), then the wait for the device.  After a failed device call the
 * device is waited for too, once, before the caller's buffers go away. */
template <typename Order>
int
download_records (int rc, const uint64_t *d_count, const ACMRecord *d_rec, ACMRecord *records, uint64_t capacity, uint64_t *n_found,
                  const BatchDownload *batch, Order order) {
  uint64_t found = 0;
  if (!rc) {
    HOST_TRY (hipMemcpy (&found, d_count, 8, hipMemcpyDeviceToHost));
    *n_found = found;
    if (found > capacity) {
      if (batch && batch->first_on_overflow && batch->first) /* (complete on the device whatever the room) */
        HOST_TRY (hipMemcpy (batch->first, batch->d_first, (batch->n_texts + 1) * 8, hipMemcpyDeviceToHost));
      return ACM_GPU_E_OVERFLOW;
    }
    rc = order (found);
  }
  if (rc) {
    (void)hipDeviceSynchronize ();
    return rc;
  }
  if (found)
    HOST_TRY (hipMemcpy (records, d_rec, found * 16, hipMemcpyDeviceToHost));
  if (batch && found && batch->text_id)
    HOST_TRY (hipMemcpy (batch->text_id, batch->d_text_id, found * 4, hipMemcpyDeviceToHost));
  if (batch && batch->first)
    HOST_TRY (hipMemcpy (batch->first, batch->d_first, (batch->n_texts + 1) * 8, hipMemcpyDeviceToHost));
  HOST_TRY (hipDeviceSynchronize ());
  return ACM_GPU_OK;
}

int
download_records (int rc, const uint64_t *d_count, const ACMRecord *d_rec, ACMRecord *records, uint64_t capacity, uint64_t *n_found,
                  const BatchDownload *batch = nullptr) {
  return download_records (rc, d_count, d_rec, records, capacity, n_found, batch, [] (uint64_t) { return (int)ACM_GPU_OK; });
}

/* ---- the steps the host conveniences share, one copy of each.
 * The text of a call on the device, in a block of `temps` */
hipError_t
upload_text (DeviceTemps &temps, const ACMPlan *plan, const void *text, uint64_t n_symbols, void **d_text) {
  const size_t tbytes = (size_t)n_symbols * plan->text_sym_bytes;
  const hipError_t e = temps.get (d_text, tbytes);
  return e != hipSuccess || !tbytes ? e : hipMemcpy (*d_text, text, tbytes, hipMemcpyHostToDevice);
}

/* the same for offsets[0 .. n_texts] of a batch */
hipError_t
upload_offsets (DeviceTemps &temps, const uint64_t *offsets, uint64_t n_texts, uint64_t **d_off) {
  const hipError_t e = temps.get (d_off, (n_texts + 1) * 8);
  return e != hipSuccess ? e : hipMemcpy (*d_off, offsets, (n_texts + 1) * 8, hipMemcpyHostToDevice);
}

/* behind a device call that gave rc: with check_status the plan's error word is read after a call that succeeded (which
 * waits for the device); after a failure the device is waited for, once, before the caller's buffers go away */
int
settle (ACMPlan *plan, int rc, bool check_status) {
  if (!rc && check_status)
    rc = acm_gpu_plan_status (plan);
  if (rc)
    (void)hipDeviceSynchronize ();
  return rc;
}

/* the record room of the calls whose caller gives none and sees no record overflow (replace, tokens): the exact number
 * of matches, counted first into d_count and brought down in one round trip (below acm_gpu_scan_select_device's limit) */
int
count_first (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t *d_count, uint64_t *matches) {
  if (const int rc = settle (plan, acm_gpu_count_device (plan, d_text, n_symbols, 0, d_count, nullptr), false))
    return rc;
  HOST_TRY (hipMemcpy (matches, d_count, 8, hipMemcpyDeviceToHost));
  return *matches >= (1ull << 31) ? ACM_GPU_E_ARG : ACM_GPU_OK;
}

/* offsets[0 .. n_texts] of a batch on the host: first 0, non-decreasing (the last is the number of symbols) */
bool
batch_offsets_ok (const uint64_t *offsets, uint64_t n_texts) {
  if (!offsets || offsets[0] != 0)
    return false;
  for (uint64_t t = 0; t < n_texts; t++)
    if (offsets[t] > offsets[t + 1])
      return false;
  return true;
}

/* the anchored records call takes fewer texts than this: hipCUB's sum counts its n_texts + 1 items in an int */
constexpr uint64_t ANCHORED_MOST_TEXTS = (1ull << 31) - 1;

/* a batch's arguments: fewer than `limit` texts, offsets[] as above, a text where there are symbols */
bool
batch_args_ok (const void *text, const uint64_t *offsets, uint64_t n_texts, uint64_t limit) {
  return n_texts < limit && batch_offsets_ok (offsets, n_texts) && (!offsets[n_texts] || text);
}

/* the device calls' shared checks.  A buffer of n symbols of sb bytes on the device (a text, an
 * output): on the symbols' grid, its bytes countable in 56 bits */
bool
symbols_ok (const void *d, uint64_t n, uint32_t sb) {
  return reinterpret_cast<uintptr_t> (d) % sb == 0 && n < (1ull << 56) / sb;
}

/* an output of out_capacity symbols built from the text beside it: the two do not overlap */
bool
apart (const void *d_text, uint64_t n_symbols, const void *d_out, uint64_t out_capacity, uint32_t sb) {
  const uintptr_t t0 = reinterpret_cast<uintptr_t> (d_text), o0 = reinterpret_cast<uintptr_t> (d_out);
  return !(n_symbols && out_capacity && t0 < o0 + out_capacity * sb && o0 < t0 + n_symbols * sb);
}

/* the windowed calls (tally, grep, tally_batch): windows of whole 16-symbol groups, a record room below 2^31 */
bool
window_ok (uint64_t window_symbols, uint64_t capacity) {
  return window_symbols != 0 && window_symbols % 16 == 0 && capacity != 0 && capacity < (1ull << 31);
}

/* where offsets[] may be NULL (one text) and the number of symbols is given beside it: fewer than 2^31 texts, which end there */
bool
optional_offsets_ok (const uint64_t *offsets, uint64_t n_texts, uint64_t n_symbols) {
  return !offsets || (n_texts < (1ull << 31) && batch_offsets_ok (offsets, n_texts) && offsets[n_texts] == n_symbols);
}

/* SPLIT's delimiters and flags */
bool
split_args_ok (const void *delims, uint32_t n_delims, uint32_t flags) {
  return delims && n_delims != 0 && n_delims <= ACM_SPLIT_MAX_DELIMS && flags <= ACM_SPLIT_RUNS;
}

/* acm_gpu_scan_host over `prefix` (n_prefix symbols, may be none) followed by `text`: the two are
 * uploaded side by side, so that acm_scan_from need not copy its text on the host */
int
scan_host_prefixed (ACMPlan *plan, const void *prefix, uint64_t n_prefix, const void *text, uint64_t n_text, uint64_t emit_from, uint64_t pos_base,
                    ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  if (!plan || !n_found || (n_text && !text) || (n_prefix && !prefix) || (capacity && !records))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const uint64_t n_symbols = n_prefix + n_text;
  const size_t tbytes = (size_t)n_symbols * plan->text_sym_bytes, pbytes = (size_t)n_prefix * plan->text_sym_bytes;
  DeviceTemps temps;
  unsigned char *d_text = nullptr;
  uint64_t *d_count = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (temps.get (&d_text, tbytes));
  HOST_TRY (temps.get (&d_count, 8));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  if (pbytes)
    HOST_TRY (hipMemcpy (d_text, prefix, pbytes, hipMemcpyHostToDevice));
  if (tbytes > pbytes)
    HOST_TRY (hipMemcpy (d_text + pbytes, text, tbytes - pbytes, hipMemcpyHostToDevice));
  const int rc = acm_gpu_scan_device (plan, d_text, n_symbols, emit_from, pos_base, d_rec, capacity, d_count, nullptr);
  return download_records (rc, d_count, d_rec, records, capacity, n_found, nullptr, [&] (uint64_t found) -> int {
    if (found <= 1)
      return ACM_GPU_OK;
    const size_t tb = acm_gpu_order_tmp_bytes (plan, found, n_symbols);
    void *d_tmp = nullptr;
    HOST_TRY (temps.get (&d_tmp, tb));
    return acm_gpu_order_records_device (plan, d_rec, found, pos_base, n_symbols, d_tmp, tb, nullptr);
  });
}
} // namespace

extern "C" int
acm_gpu_scan_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t emit_from, uint64_t pos_base,
                   ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  return scan_host_prefixed (plan, nullptr, 0, text, n_symbols, emit_from, pos_base, records, capacity, n_found);
}

/* ------------------------------------------------------------------ batch scans (include/acm_gpu.h, dev_batch.h)
 * The ordered scan of the concatenation into the caller's scratch, then the pass over its records:
 * those that lie inside one text go to d_records, with their text beside them. */
namespace {
/* what batch_carve derives beside K's pointers */
struct BatchRoom {
  uint32_t *tile_begin = nullptr; /* K.tile_begin, for the sum that writes it */
  CubRoom cub;
  ACMRecord *ordered = nullptr; /* the ordered scan's records and its scratch */
  unsigned char *ord = nullptr;
  size_t ord_bytes = 0;
};
BatchRoom
batch_carve (Carve &c, const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, BatchK &K) {
  BatchRoom R;
  K.n_blocks = (n_symbols >> BATCH_BLOCK_LOG2) + 2;
  K.n_tiles = (capacity + BATCH_TILE - 1) / BATCH_TILE;
  R.ord_bytes = acm_gpu_scan_ordered_tmp_bytes (plan, capacity, n_symbols);
  K.ctl = c.take<BatchCtl> (1);
  K.index = c.take<uint32_t> (K.n_blocks);
  K.tile_count = c.take<uint32_t> (K.n_tiles + 1);
  K.tile_begin = R.tile_begin = c.take<uint32_t> (K.n_tiles + 1);
  R.cub = cub_room (c, K.n_tiles + 1, 0);
  K.in = R.ordered = c.take<ACMRecord> (capacity ? capacity : 1);
  R.ord = c.take (R.ord_bytes);
  return R;
}

/* grid-stride kernels: never more blocks than keep the chip busy.  The kernels that also walk
 * offsets[] are sized by the positions; a batch of many texts over few symbols (mostly empty texts)
 * gets the full capped grid instead -- one size, whatever the number of texts */
dim3
batch_grid (const ACMPlan *plan, uint64_t by_positions, uint64_t n_texts) {
  const uint64_t many_texts = n_texts >= (1ull << 16) ? (uint64_t)plan->cu_count * 8 : 1;
  return capped_grid (plan, std::max (by_positions, many_texts));
}

/* the first step of the batch and flow scans, of grep and of tally_batch: for every block of
 * positions the text it begins in, into index[n_blocks], and the check of offsets[], whose verdict
 * goes to ctl->bad and to the plan's error word.  pre_bad: a flow scan's own verdict (BatchK) */
int
batch_index (const ACMPlan *plan, const uint64_t *d_offsets, uint64_t n_texts, uint64_t n_symbols, uint32_t *index, uint64_t n_blocks, BatchCtl *ctl,
             unsigned int *error, hipStream_t st, const unsigned int *pre_bad = nullptr) {
  BatchK B{};
  B.offsets = d_offsets;
  B.n_texts = n_texts;
  B.n_symbols = n_symbols;
  B.index = index;
  B.n_blocks = n_blocks;
  B.ctl = ctl;
  B.error = error;
  B.pre_bad = pre_bad;
  /* (the index goes by the positions, the check of offsets[] by a grid-stride loop of the same launch) */
  const dim3 grid = batch_grid (plan, (n_blocks + BATCH_THREADS - 1) / BATCH_THREADS, n_texts);
  HIP_TRY (pre_bad ? launch (batch_index_kernel<true>, grid, dim3 (BATCH_THREADS), 0, st, B)
                   : launch (batch_index_kernel<false>, grid, dim3 (BATCH_THREADS), 0, st, B));
  return ACM_GPU_OK;
}
} // namespace

extern "C" size_t
acm_gpu_scan_batch_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: the index goes by blocks of positions) */
  if (!plan || capacity >= (1ull << 31))
    return 0;
  Carve c;
  BatchK K{};
  batch_carve (c, plan, capacity, n_symbols, K);
  return c.total ();
}

namespace {
/* flow scans (dev_flows.h): the batch is an expanded buffer whose texts begin with carried symbols */
struct BatchHeads {
  const uint32_t *head;        /* [n_texts] carried symbols in front of every text */
  const uint64_t *base;        /* [n_real + 1] the texts' offsets in the caller's buffer */
  uint64_t n_real;             /* texts that report (the rest is fill) */
  const unsigned int *pre_bad; /* the caller's own checks have failed */
};

/* a batch of no texts: no symbol, and a zero in every output the caller gave (its counts, the first
 * entry of its row pointers) */
int
empty_batch (ACMPlan *plan, uint64_t n_symbols, std::initializer_list<uint64_t *> outputs, hipStream_t st) {
  if (n_symbols)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  for (uint64_t *d : outputs)
    if (d)
      HIP_TRY (hipMemsetAsync (d, 0, 8, st));
  return ACM_GPU_OK;
}

/* acm_gpu_scan_batch_device; HEADS: what the flow scan runs behind its gather pass */
template <bool HEADS>
int
batch_scan (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, ACMRecord *d_records,
            uint32_t *d_text_id, uint64_t *d_first, uint64_t capacity, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream,
            const BatchHeads *heads) {
  if (!plan || !d_count || n_texts >= (1ull << 32) || capacity >= (1ull << 31) || (n_symbols && !d_text) || (capacity && !d_records))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0)
    return empty_batch (plan, n_symbols, { d_count, d_first }, st);
  Carve carve (d_tmp);
  BatchK K{};
  const BatchRoom L = batch_carve (carve, plan, capacity, n_symbols, K);
  if (!d_offsets || !d_tmp || tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  int rc = acm_gpu_scan_ordered_device (plan, d_text, n_symbols, 0, 0, L.ordered, capacity, d_count, L.ord, L.ord_bytes, stream);
  if (rc)
    return rc;
  K.capacity = capacity;
  K.n_dev = reinterpret_cast<const unsigned long long *> (d_count);
  K.offsets = d_offsets;
  K.n_texts = n_texts;
  K.n_symbols = n_symbols;
  K.out = d_records;
  K.text_id = d_text_id;
  K.first = d_first;
  K.d_count = reinterpret_cast<unsigned long long *> (d_count);
  K.error = error_word (plan);
  if (HEADS) {
    K.head = heads->head;
    K.base = heads->base;
    K.n_real = heads->n_real;
    K.pre_bad = heads->pre_bad;
  }
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (BatchCtl), st));
  if (const int bad = batch_index (plan, d_offsets, n_texts, n_symbols, K.index, K.n_blocks, K.ctl, K.error, st, HEADS ? heads->pre_bad : nullptr))
    return bad;
  HIP_TRY (launch (batch_filter_kernel<false, HEADS>, capped_grid (plan, K.n_tiles + 1), dim3 (BATCH_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.tile_count, L.tile_begin, K.n_tiles + 1, st));
  HIP_TRY (launch (batch_filter_kernel<true, HEADS>, capped_grid (plan, K.n_tiles + 1), dim3 (BATCH_THREADS), 0, st, K));
  HIP_TRY (launch (batch_first_kernel<HEADS>, batch_grid (plan, K.n_blocks / 4 + 1, n_texts), dim3 (BATCH_THREADS), 0, st, K));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_scan_batch_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts,
                           ACMRecord *d_records, uint32_t *d_text_id, uint64_t *d_first, uint64_t capacity, uint64_t *d_count, void *d_tmp,
                           size_t tmp_bytes, void *stream) {
  return batch_scan<false> (plan, d_text, n_symbols, d_offsets, n_texts, d_records, d_text_id, d_first, capacity, d_count, d_tmp, tmp_bytes, stream,
                            nullptr);
}

namespace {
/* acm_gpu_scan_batch_host and, with `flows` (and maybe the texts' flow ids), acm_gpu_scan_flows_host
 * behind their argument checks: everything up, the device call, everything down */
int
batch_host (ACMPlan *plan, ACMFlows *flows, const void *text, uint64_t n_symbols, const uint64_t *offsets, const uint32_t *flow, uint64_t n_texts,
            ACMRecord *records, uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  HIP_TRY (hipSetDevice (plan->device));
  const size_t tmp_bytes = flows ? acm_gpu_scan_flows_tmp_bytes (plan, flows, capacity, n_symbols, n_texts)
                                 : acm_gpu_scan_batch_tmp_bytes (plan, capacity, n_symbols, n_texts);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_off = nullptr, *d_count = nullptr, *d_first = nullptr;
  uint32_t *d_flow = nullptr, *d_tid = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  if (flows)
    HOST_TRY (temps.get (&d_flow, n_texts * 4));
  HOST_TRY (temps.get (&d_count, 8));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  HOST_TRY (temps.get (&d_tid, capacity * 4));
  HOST_TRY (temps.get (&d_first, (n_texts + 1) * 8));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  if (flow && n_texts)
    HOST_TRY (hipMemcpy (d_flow, flow, n_texts * 4, hipMemcpyHostToDevice));
  const int rc = flows ? acm_gpu_scan_flows_device (plan, flows, d_text, n_symbols, d_off, flow ? d_flow : nullptr, n_texts, d_rec, d_tid, d_first, capacity,
                                                    d_count, d_tmp, tmp_bytes, nullptr)
                       : acm_gpu_scan_batch_device (plan, d_text, n_symbols, d_off, n_texts, d_rec, d_tid, d_first, capacity, d_count, d_tmp, tmp_bytes,
                                                    nullptr);
  const BatchDownload down = { text_id, d_tid, first, d_first, n_texts };
  return download_records (rc, d_count, d_rec, records, capacity, n_found, &down);
}
} // namespace

extern "C" int
acm_gpu_scan_batch_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, ACMRecord *records, uint32_t *text_id,
                         uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  if (!plan || !n_found || capacity >= (1ull << 31) || (capacity && !records) || !batch_args_ok (text, offsets, n_texts, 1ull << 32))
    return ACM_GPU_E_ARG;
  return batch_host (plan, nullptr, text, offsets[n_texts], offsets, nullptr, n_texts, records, text_id, first, capacity, n_found);
}

/* ------------------------------------------------------------------ flow scans (include/acm_gpu.h, dev_flows.h)
 * Per-flow state on the device and the passes around the batch scan that use it. */
struct ACMFlows {
  ACMPlan *plan = nullptr;
  int device = 0;
  uint64_t n_flows = 0;
  uint32_t sb = 1;           /* bytes per symbol of the caller's text */
  uint32_t slot_symbols = 0; /* a slot holds this many: lmax - 1 at creation, rounded up to whole 16 bytes */
  uint32_t slot_bytes = 16;
  unsigned char *d_carry = nullptr; /* [n_flows] slots */
  uint32_t *d_len = nullptr;        /* [n_flows] symbols each slot holds */
  uint32_t *d_claim = nullptr;      /* [n_flows] sequence number of the last call the flow took part in */
  uint32_t seq = 0;
};

namespace {
/* symbols of a full carry: the longest keyword of the plan and of its delta, less one */
uint32_t
flows_keep (const ACMPlan *p) {
  const uint32_t lmax = plan_lmax (p);
  return lmax > 1 ? lmax - 1 : 0;
}

struct HeadTo64 {
  __host__ __device__ uint64_t operator() (uint32_t v) const { return v; }
};
using HeadIterator = hipcub::TransformInputIterator<uint64_t, HeadTo64, const uint32_t *>;

/* what flows_carve derives beside F's pointers */
struct FlowsRoom {
  uint64_t *head_sum = nullptr; /* F.head_sum, for the sum that writes it */
  CubRoom cub;
  unsigned char *batch = nullptr; /* the batch scan's scratch */
  size_t batch_bytes = 0;
};
FlowsRoom
flows_carve (Carve &c, const ACMPlan *plan, const ACMFlows *flows, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts, FlowsK &F) {
  FlowsRoom R;
  F.n_expanded = n_symbols + n_texts * flows_keep (plan); /* every text behind a full carry: the worst case */
  (void)hipcub::DeviceScan::ExclusiveSum (nullptr, R.cub.bytes, HeadIterator (static_cast<const uint32_t *> (nullptr), HeadTo64 ()), static_cast<uint64_t *> (nullptr), (int)(n_texts + 1), nullptr);
  Carve sized;
  BatchK B{};
  batch_carve (sized, plan, capacity, F.n_expanded, B);
  R.batch_bytes = sized.total ();
  F.ctl = c.take<FlowsCtl> (1);
  F.head = c.take<uint32_t> (n_texts + 1);
  F.head_sum = R.head_sum = c.take<uint64_t> (n_texts + 1);
  F.xoff = c.take<uint64_t> (n_texts + 2);
  R.cub.at = c.take (R.cub.bytes + 16);
  F.expanded = c.take (F.n_expanded * flows->sb + 256);
  R.batch = c.take (R.batch_bytes);
  Carve inner (R.batch); /* (the batch scan's control block, where batch_scan will put it) */
  batch_carve (inner, plan, capacity, F.n_expanded, B);
  F.batch = B.ctl;
  return R;
}

uint32_t
log2_ceil_capped (uint64_t x, uint32_t most) {
  uint32_t l = 0;
  while (l < most && (1ull << l) < x)
    l++;
  return l;
}
} // namespace

extern "C" int
acm_gpu_flows_create (ACMPlan *plan, uint64_t n_flows, ACMFlows **out) {
  if (!plan || !out || n_flows == 0 || n_flows >= (1ull << 32))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  ACMFlows *f = new (std::nothrow) ACMFlows ();
  if (!f)
    return ACM_GPU_E_NOMEM;
  f->plan = plan;
  f->device = plan->device;
  f->n_flows = n_flows;
  f->sb = plan->text_sym_bytes;
  f->slot_bytes = (uint32_t)(((size_t)flows_keep (plan) * f->sb + 15) / 16 * 16);
  if (f->slot_bytes == 0)
    f->slot_bytes = 16;
  f->slot_symbols = f->slot_bytes / f->sb;
  const bool ok = hipMalloc (reinterpret_cast<void **> (&f->d_carry), (size_t)n_flows * f->slot_bytes) == hipSuccess &&
                  hipMalloc (reinterpret_cast<void **> (&f->d_len), (size_t)n_flows * 4) == hipSuccess &&
                  hipMalloc (reinterpret_cast<void **> (&f->d_claim), (size_t)n_flows * 4) == hipSuccess &&
                  hipMemset (f->d_len, 0, (size_t)n_flows * 4) == hipSuccess && hipMemset (f->d_claim, 0, (size_t)n_flows * 4) == hipSuccess &&
                  hipDeviceSynchronize () == hipSuccess;
  if (!ok) {
    acm_gpu_flows_destroy (f);
    return ACM_GPU_E_NOMEM;
  }
  *out = f;
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_flows_destroy (ACMFlows *f) {
  if (!f)
    return;
  (void)hipSetDevice (f->device);
  for (void *d : { static_cast<void *> (f->d_carry), static_cast<void *> (f->d_len), static_cast<void *> (f->d_claim) })
    if (d)
      (void)hipFree (d);
  delete f;
}

extern "C" int
acm_gpu_flows_reset (ACMFlows *f, const uint32_t *d_flow_ids, uint64_t n, void *stream) {
  if (!f)
    return ACM_GPU_E_ARG;
  const uint64_t items = d_flow_ids ? n : f->n_flows;
  if (items == 0)
    return ACM_GPU_OK;
  ACMPlan *plan = f->plan;
  HIP_TRY (hipSetDevice (plan->device));
  HIP_TRY (launch (flows_reset_kernel, capped_grid (plan, (items + FLOWS_THREADS - 1) / FLOWS_THREADS), dim3 (FLOWS_THREADS), 0,
                   static_cast<hipStream_t> (stream), f->d_len, f->n_flows, d_flow_ids, n, error_word (plan)));
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_scan_flows_tmp_bytes (const ACMPlan *plan, const ACMFlows *flows, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || !flows || flows->plan != plan || capacity >= (1ull << 31) || n_texts >= (1ull << 31))
    return 0;
  Carve c;
  FlowsK F{};
  flows_carve (c, plan, flows, capacity, n_symbols, n_texts, F);
  return c.total ();
}

extern "C" int
acm_gpu_scan_flows_device (ACMPlan *plan, ACMFlows *flows, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, const uint32_t *d_flow,
                           uint64_t n_texts, ACMRecord *d_records, uint32_t *d_text_id, uint64_t *d_first, uint64_t capacity, uint64_t *d_count,
                           void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !flows || flows->plan != plan || !d_count || n_texts >= (1ull << 31) || capacity >= (1ull << 31) || (n_symbols && !d_text) ||
      (capacity && !d_records))
    return ACM_GPU_E_ARG;
  const uint32_t keep = flows_keep (plan);
  if (keep > flows->slot_symbols) /* an update has brought a keyword longer than the slots were made for: never a short carry */
    return ACM_GPU_E_ARG;
  if (!d_flow && n_texts > flows->n_flows)
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0)
    return empty_batch (plan, n_symbols, { d_count, d_first }, st);
  Carve carve (d_tmp);
  FlowsK F{};
  const FlowsRoom L = flows_carve (carve, plan, flows, capacity, n_symbols, n_texts, F);
  if (!d_offsets || !d_tmp || tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  if (++flows->seq == 0) { /* the sequence numbers have gone round: no claim of an old call may look like a new one */
    HIP_TRY (hipMemsetAsync (flows->d_claim, 0, (size_t)flows->n_flows * 4, st));
    flows->seq = 1;
  }
  F.text = static_cast<const unsigned char *> (d_text);
  F.offsets = d_offsets;
  F.flow = d_flow;
  F.n_texts = n_texts;
  F.n_symbols = n_symbols;
  F.n_flows = flows->n_flows;
  F.sb = flows->sb;
  F.keep = keep;
  F.slot_bytes = flows->slot_bytes;
  F.carry = flows->d_carry;
  F.carry_len = flows->d_len;
  F.claim = flows->d_claim;
  F.seq = flows->seq;
  F.error = error_word (plan);
  /* grid-stride kernels with capped grids: one launch size whatever the number of texts and flows */
  const uint64_t per_text = (n_texts + 2 + FLOWS_THREADS - 1) / FLOWS_THREADS;
  HIP_TRY (hipMemsetAsync (F.ctl, 0, sizeof (FlowsCtl), st));
  HIP_TRY (launch (flows_check_kernel, capped_grid (plan, per_text), dim3 (FLOWS_THREADS), 0, st, F));
  HIP_TRY (launch (flows_head_kernel, capped_grid (plan, per_text), dim3 (FLOWS_THREADS), 0, st, F));
  HIP_TRY (exclusive_sum (L.cub, HeadIterator (F.head, HeadTo64 ()), L.head_sum, n_texts + 1, st));
  HIP_TRY (launch (flows_xoff_kernel, capped_grid (plan, per_text), dim3 (FLOWS_THREADS), 0, st, F));
  /* the gather: lanes per text by the mean length of a text, 16 bytes a lane and step */
  F.group_log2 = log2_ceil_capped ((n_symbols * F.sb / n_texts + 15) / 16, 6);
  const uint64_t gather_blocks = std::max (((n_texts << F.group_log2) + FLOWS_THREADS - 1) / FLOWS_THREADS, n_texts * keep * F.sb / 16 / FLOWS_THREADS + 1);
  HIP_TRY (launch (flows_gather_kernel, capped_grid (plan, gather_blocks), dim3 (FLOWS_THREADS), 0, st, F));
  BatchHeads H{ F.head, d_offsets, n_texts, &F.ctl->bad };
  const int rc = batch_scan<true> (plan, F.expanded, F.n_expanded, F.xoff, n_texts + 1, d_records, d_text_id, d_first, capacity, d_count, L.batch,
                                   L.batch_bytes, stream, &H);
  if (rc)
    return rc;
  F.group_log2 = log2_ceil_capped (flows->slot_bytes / 16, 6);
  HIP_TRY (launch (flows_carry_kernel, capped_grid (plan, ((n_texts << F.group_log2) + FLOWS_THREADS - 1) / FLOWS_THREADS), dim3 (FLOWS_THREADS), 0, st, F));
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_scan_flows_host (ACMPlan *plan, ACMFlows *flows, const void *text, uint64_t n_symbols, const uint64_t *offsets, const uint32_t *flow,
                         uint64_t n_texts, ACMRecord *records, uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  if (!plan || !flows || flows->plan != plan || !n_found || capacity >= (1ull << 31) || (capacity && !records) ||
      !batch_args_ok (text, offsets, n_texts, 1ull << 31) || offsets[n_texts] != n_symbols)
    return ACM_GPU_E_ARG;
  /* the flow ids, checked here as the device checks them: below n_flows, none twice */
  if (!flow && n_texts > flows->n_flows)
    return ACM_GPU_E_ARG;
  if (flow) {
    std::vector<uint32_t> ids (flow, flow + n_texts);
    std::sort (ids.begin (), ids.end ());
    if ((n_texts && ids.back () >= flows->n_flows) || std::adjacent_find (ids.begin (), ids.end ()) != ids.end ())
      return ACM_GPU_E_ARG;
  }
  return batch_host (plan, flows, text, n_symbols, offsets, flow, n_texts, records, text_id, first, capacity, n_found);
}

/* ------------------------------------------------------------------ per-keyword tallies (include/acm_gpu.h, dev_tally.h)
 * The record scan of the text, window by window into the caller's scratch, and a histogram pass
 * over every window's records; the caller's counters take the sums at the end, all or nothing. */
namespace {
/* what tally_carve derives beside K's pointers */
struct TallyRoom {
  size_t zero_bytes = 0; /* control words, histogram, count: the head of the scratch, cleared in front of every call */
  uint64_t *d_count = nullptr;
  ACMRecord *rec = nullptr;
};
TallyRoom
tally_carve (Carve &c, const ACMPlan *plan, uint64_t capacity, TallyK &K) {
  TallyRoom R;
  K.ctl = c.take<TallyCtl> (1);
  K.hist = c.take<unsigned long long> ((size_t)plan->covered_keywords + 1);
  R.d_count = c.take<uint64_t> (1);
  R.zero_bytes = c.boundary (); /* (up to where the records begin) */
  R.rec = c.take<ACMRecord> ((size_t)capacity);
  return R;
}

/* ACM_GPU_TALLY=global: every plan takes the form of the big dictionaries (experiments, tests) */
bool
tally_lds_form (const ACMPlan *plan) {
  const bool global = getenv ("ACM_GPU_TALLY") && strcmp (getenv ("ACM_GPU_TALLY"), "global") == 0;
  return !global && plan->covered_keywords <= TALLY_LDS_KEYWORDS;
}

/* the window walk of acm_gpu_tally_device and acm_gpu_grep_device: window w owns the matches that
 * end in it and starts from the root lmax - 1 symbols early, rounded down to a 16-byte boundary of
 * the text (acm_gpu_multi_shard_bounds' rule: the kernels keep their alignment).  Every window is
 * scanned into `rec`, its count into d_count; behind (read begin) queues what the caller does with
 * the records, whose positions are relative to the window's read begin. */
template <typename Behind>
int
scan_windows (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from, uint64_t window_symbols, ACMRecord *rec, uint64_t capacity,
              uint64_t *d_count, hipStream_t st, Behind behind) {
  const uint32_t sb = plan->text_sym_bytes;
  const uint64_t per16 = 16 / sb ? 16 / sb : 1, warm = flows_keep (plan);
  for (uint64_t wb = emit_from / window_symbols * window_symbols; wb < n_symbols; wb += window_symbols) {
    const uint64_t we = n_symbols - wb > window_symbols ? wb + window_symbols : n_symbols;
    const uint64_t ef = emit_from > wb ? emit_from : wb;
    const uint64_t rb = (wb > warm ? wb - warm : 0) / per16 * per16;
    int rc = scan_plan<false> (plan, static_cast<const unsigned char *> (d_text) + rb * sb, we - rb, ef - rb, 0, rec, capacity, d_count, st);
    if (!rc)
      rc = behind (rb);
    if (rc)
      return rc;
  }
  return ACM_GPU_OK;
}

/* M of the capacity bound: most records one position can have, the plan's and its delta's.  A
 * start-parallel plan that is edited in place does not keep finfo.max_outputs up to date: the
 * keywords that end at one position have different lengths, so lmax bounds their number. */
uint64_t
tally_max_outputs (const ACMPlan *plan) {
  uint64_t m = 0;
  for (const ACMPlan *p : { plan, static_cast<const ACMPlan *> (plan->delta) })
    if (p)
      m += p->mir ? std::min (p->finfo.lmax, p->finfo.n_keywords) : p->finfo.max_outputs;
  return m ? m : 1;
}

/* the window and the record room of the windowed host calls (tally, grep, tally_batch): windows of
 * 32 Mi symbols, room for 2 Mi records (32 MiB) -- one match per 16 symbols; the environment can
 * set another room, in records (tests of the second attempt) */
struct RecordRoom {
  uint64_t window, capacity;
  bool shrunk;
};

RecordRoom
tally_room (const ACMPlan *plan, uint64_t n_symbols) {
  RecordRoom R = { 1ull << 25, 1ull << 21, false };
  if (const char *e = getenv ("ACM_GPU_TALLY_CAPACITY")) {
    const long long said = atoll (e);
    if (said > 0 && (uint64_t)said < (1ull << 31))
      R.capacity = (uint64_t)said;
  }
  /* (a short text cannot have more than n x M records) */
  const uint64_t m = tally_max_outputs (plan);
  if (n_symbols < (1ull << 31) / m && n_symbols * m < R.capacity)
    R.capacity = n_symbols ? n_symbols * m : 1;
  return R;
}

/* the second attempt, behind a window that had more records than the room: a window of W symbols
 * has at most W x M records, so this one cannot overflow.  false: it did all the same (never expected) */
bool
tally_room_shrink (const ACMPlan *plan, RecordRoom *R) {
  if (R->shrunk)
    return false;
  R->shrunk = true;
  const uint64_t m = tally_max_outputs (plan);
  if (R->capacity / m < 16)
    R->capacity = 16 * m;
  R->window = R->capacity / m / 16 * 16;
  return true;
}
} // namespace

extern "C" int
acm_gpu_tally_form (const ACMPlan *plan) {
  if (!plan)
    return ACM_GPU_E_ARG;
  return tally_lds_form (plan) ? ACM_GPU_TALLY_FORM_LDS : ACM_GPU_TALLY_FORM_GLOBAL;
}

extern "C" uint64_t
acm_gpu_tally_keywords (const ACMPlan *plan) {
  return plan ? plan->covered_keywords : 0;
}

extern "C" size_t
acm_gpu_tally_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity) {
  (void)window_symbols; /* (what a window's scan needs beside its records belongs to the plan) */
  if (!plan || capacity == 0 || capacity >= (1ull << 31))
    return 0;
  Carve c;
  TallyK K{};
  tally_carve (c, plan, capacity, K);
  return c.total ();
}

extern "C" int
acm_gpu_tally_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t emit_from, uint64_t *d_tally, uint64_t n_keywords,
                      uint64_t window_symbols, uint64_t capacity, uint64_t *d_total, uint64_t *d_need, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_tally || !d_total || !d_need || !d_tmp || (n_symbols && !d_text) || !window_ok (window_symbols, capacity) ||
      n_keywords < plan->covered_keywords)
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  TallyK K{}; /* the finish pass'; the window passes add the records to a copy */
  const TallyRoom L = tally_carve (carve, plan, capacity, K);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  HIP_TRY (hipMemsetAsync (d_total, 0, 8, st));
  K.capacity = capacity;
  K.n_keywords = plan->covered_keywords;

  const int rc = scan_windows (plan, d_text, n_symbols, emit_from, window_symbols, L.rec, capacity, L.d_count, st, [&] (uint64_t) -> int {
    TallyK W = K;
    W.rec = L.rec;
    W.n_dev = reinterpret_cast<const unsigned long long *> (L.d_count);
    W.error = error_word (plan);
    /* grid-stride, two blocks per CU (what the LDS form's counters allow), whatever the scan found */
    const dim3 grid ((uint32_t)plan->cu_count * 2);
    HIP_TRY (tally_lds_form (plan) ? launch (tally_records_kernel<true>, grid, dim3 (TALLY_THREADS), (size_t)W.n_keywords * 4, st, W)
                                   : launch (tally_records_kernel<false>, grid, dim3 (TALLY_THREADS), 0, st, W));
    return ACM_GPU_OK;
  });
  if (rc)
    return rc;
  K.d_tally = reinterpret_cast<unsigned long long *> (d_tally);
  K.d_total = reinterpret_cast<unsigned long long *> (d_total);
  K.d_need = reinterpret_cast<unsigned long long *> (d_need);
  HIP_TRY (launch (tally_finish_kernel, capped_grid (plan, ((uint64_t)K.n_keywords + TALLY_THREADS - 1) / TALLY_THREADS), dim3 (TALLY_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_tally_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t *tally, uint64_t n_keywords, uint64_t *total) {
  if (!plan || !tally || (n_symbols && !text) || n_keywords < plan->covered_keywords)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  RecordRoom room = tally_room (plan, n_symbols);
  const uint32_t kw = plan->covered_keywords;
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_tally = nullptr, *d_out = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_tally, ((size_t)kw + 1) * 8));
  HOST_TRY (temps.get (&d_out, 16)); /* total, need */
  HOST_TRY (hipMemset (d_tally, 0, ((size_t)kw + 1) * 8));
  uint64_t out[2] = { 0, 0 };
  for (;;) {
    const size_t tmp_bytes = acm_gpu_tally_tmp_bytes (plan, room.window, room.capacity);
    HOST_TRY (temps.get (&d_tmp, tmp_bytes));
    /* (the one windowed call that does not read the plan's error word) */
    if (const int rc = settle (plan, acm_gpu_tally_device (plan, d_text, n_symbols, 0, d_tally, kw, room.window, room.capacity, d_out, d_out + 1, d_tmp,
                                                           tmp_bytes, nullptr), false))
      return rc;
    HOST_TRY (hipMemcpy (out, d_out, 16, hipMemcpyDeviceToHost));
    HOST_TRY (temps.release (d_tmp)); /* (the second attempt's is another size) */
    if (out[1] <= room.capacity)
      break;
    if (!tally_room_shrink (plan, &room))
      return ACM_GPU_E_INTERNAL;
  }
  std::vector<uint64_t> add ((size_t)kw + 1);
  HOST_TRY (hipMemcpy (add.data (), d_tally, (size_t)kw * 8, hipMemcpyDeviceToHost));
  HOST_TRY (hipDeviceSynchronize ());
  for (uint32_t k = 0; k < kw; k++)
    tally[k] += add[k];
  if (total)
    *total = out[0];
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ grep over a batch (include/acm_gpu.h, dev_grep.h)
 * The record scan of the buffer, window by window into the caller's scratch, a pass over every
 * window's records that counts them per text, then the kept texts' ids, their offsets in the
 * output and the output itself. */
namespace {
/* what grep_carve derives beside K's pointers */
struct GrepRoom {
  uint64_t n_blocks = 0;
  size_t zero_bytes = 0; /* control words, count, hit counters: the head of the scratch, cleared in front of every call */
  uint64_t *d_count = nullptr;
  ACMRecord *rec = nullptr; /* K's, for the passes that write them */
  uint32_t *index = nullptr, *tile_kept_begin = nullptr;
  long long *tile_sym = nullptr, *tile_sym_begin = nullptr;
  CubRoom cub;
};
GrepRoom
grep_carve (Carve &c, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts, GrepK &K) {
  GrepRoom R;
  R.n_blocks = (n_symbols >> BATCH_BLOCK_LOG2) + 2;
  K.n_tiles = (n_texts + GREP_TILE - 1) / GREP_TILE;
  K.ctl = c.take<GrepCtl> (1);
  R.d_count = c.take<uint64_t> (1);
  K.hits = c.take<unsigned long long> (n_texts + 1);
  R.zero_bytes = c.used;
  K.index = R.index = c.take<uint32_t> (R.n_blocks);
  K.tile_kept = c.take<uint32_t> (K.n_tiles + 1);
  K.tile_kept_begin = R.tile_kept_begin = c.take<uint32_t> (K.n_tiles + 1);
  R.tile_sym = c.take<long long> (K.n_tiles + 1);
  R.tile_sym_begin = c.take<long long> (K.n_tiles + 1);
  K.tile_sym = reinterpret_cast<unsigned long long *> (R.tile_sym);
  K.tile_sym_begin = reinterpret_cast<const unsigned long long *> (R.tile_sym_begin);
  R.cub = cub_room (c, K.n_tiles + 1, K.n_tiles + 1);
  K.kept = c.take<uint32_t> (n_texts + 1);
  K.kept_off = c.take<unsigned long long> (n_texts + 2);
  K.rec = R.rec = c.take<ACMRecord> ((size_t)capacity);
  return R;
}
} // namespace

extern "C" size_t
acm_gpu_grep_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  (void)window_symbols; /* (what a window's scan needs beside its records belongs to the plan) */
  if (!plan || capacity == 0 || capacity >= (1ull << 31) || n_texts >= (1ull << 31))
    return 0;
  Carve c;
  GrepK K{};
  grep_carve (c, capacity, n_symbols, n_texts, K);
  return c.total ();
}

extern "C" int
acm_gpu_grep_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint32_t flags,
                     uint64_t window_symbols, uint64_t capacity, uint64_t *d_hits, uint32_t *d_kept, uint64_t *d_n_kept, uint64_t *d_total,
                     uint64_t *d_need, void *d_out, uint64_t out_capacity, uint64_t *d_out_offsets, uint64_t *d_out_symbols, void *d_tmp,
                     size_t tmp_bytes, void *stream) {
  if (!plan || !d_n_kept || !d_total || !d_need || (n_symbols && !d_text) || !window_ok (window_symbols, capacity) || n_texts >= (1ull << 31) ||
      flags > ACM_GREP_INVERT || (d_out != nullptr) != (d_out_symbols != nullptr))
    return ACM_GPU_E_ARG;
  const uint32_t sb = plan->text_sym_bytes;
  if (!symbols_ok (d_text, n_symbols, sb) || !symbols_ok (d_out, out_capacity, sb) || (d_out && !apart (d_text, n_symbols, d_out, out_capacity, sb)))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0) /* (nothing kept) */
    return empty_batch (plan, n_symbols, { d_n_kept, d_total, d_need, d_out_symbols, d_out_offsets }, st);
  Carve carve (d_tmp);
  GrepK K{};
  const GrepRoom L = grep_carve (carve, capacity, n_symbols, n_texts, K);
  if (!d_offsets || !d_tmp || tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.capacity = capacity;
  K.n_dev = reinterpret_cast<const unsigned long long *> (L.d_count);
  K.offsets = d_offsets;
  K.n_texts = n_texts;
  K.n_symbols = n_symbols;
  K.flags = flags;
  K.d_hits = reinterpret_cast<unsigned long long *> (d_hits);
  K.d_kept = d_kept;
  K.d_out_offsets = reinterpret_cast<unsigned long long *> (d_out_offsets);
  K.d_n_kept = reinterpret_cast<unsigned long long *> (d_n_kept);
  K.d_total = reinterpret_cast<unsigned long long *> (d_total);
  K.d_need = reinterpret_cast<unsigned long long *> (d_need);
  K.d_out_symbols = reinterpret_cast<unsigned long long *> (d_out_symbols);
  K.text = static_cast<const unsigned char *> (d_text);
  K.out = static_cast<unsigned char *> (d_out);
  K.out_capacity = out_capacity;
  K.sb = sb;
  /* ACM_GPU_GREP_TILE=<bytes of output>: the gather's tile, a multiple of 16 (tests) */
  K.tile_words = tunable ("ACM_GPU_GREP_TILE", GREP_OUT_TILE_DEFAULT, GREP_OUT_TILE_MIN, GREP_OUT_TILE_MAX, Tune::Mult16) / 16;
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  /* 1. the index and the check of offsets[] */
  if (const int bad = batch_index (plan, d_offsets, n_texts, n_symbols, L.index, L.n_blocks, &K.ctl->batch, K.error, st))
    return bad;
  /* 2. every window's records, counted per text: the grid by the room, whatever the scan found */
  const dim3 hits_grid = capped_grid (plan, (capacity + GREP_THREADS - 1) / GREP_THREADS);
  const int rc = scan_windows (plan, d_text, n_symbols, 0, window_symbols, L.rec, capacity, L.d_count, st, [&] (uint64_t read_begin) -> int {
    K.read_begin = read_begin;
    HIP_TRY (launch (grep_hits_kernel, hits_grid, dim3 (GREP_THREADS), 0, st, K));
    return ACM_GPU_OK;
  });
  if (rc)
    return rc;
  /* 3. */
  const dim3 tiles_grid = capped_grid (plan, K.n_tiles + 1);
  HIP_TRY (launch (grep_flag_kernel<false>, tiles_grid, dim3 (GREP_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.tile_kept, L.tile_kept_begin, K.n_tiles + 1, st));
  HIP_TRY (exclusive_sum (L.cub, L.tile_sym, L.tile_sym_begin, K.n_tiles + 1, st));
  HIP_TRY (launch (grep_flag_kernel<true>, tiles_grid, dim3 (GREP_THREADS), 0, st, K));
  /* 4. the grid by the room of the output, not by what the passes found */
  if (d_out) {
    const uint64_t tiles = (out_capacity * sb + 15 + 16) / ((uint64_t)K.tile_words * 16) + 1;
    HIP_TRY (launch (grep_gather_kernel, capped_grid (plan, tiles), dim3 (GREP_THREADS), 0, st, K));
  }
  return ACM_GPU_OK;
}

namespace {
/* what acm_gpu_grep_host and acm_gpu_grep_lines_host do once the text and its offsets are on the
 * device (blocks of `temps`, which also owns what this makes): tally_room and its one repeat, the
 * downloads.  Arguments as acm_gpu_grep_host's, checked by the caller. */
int
grep_resident (ACMPlan *plan, DeviceTemps &temps, const void *d_text, uint64_t n_symbols, const uint64_t *d_off, uint64_t n_texts, uint32_t flags,
               uint64_t *hits, uint32_t *kept, uint64_t *n_kept, uint64_t *total, void *out, uint64_t out_capacity, uint64_t *out_offsets,
               uint64_t *out_symbols) {
  RecordRoom room = tally_room (plan, n_symbols);
  const uint32_t sb = plan->text_sym_bytes;
  if (!out)
    out_capacity = 0;
  void *d_tmp = nullptr, *d_out = nullptr;
  uint64_t *d_hits = nullptr, *d_out_off = nullptr, *d_res = nullptr; /* d_res: n_kept, total, need, out_symbols */
  uint32_t *d_kept = nullptr;
  HOST_TRY (temps.get (&d_hits, n_texts * 8));
  HOST_TRY (temps.get (&d_kept, n_texts * 4));
  HOST_TRY (temps.get (&d_out_off, (n_texts + 1) * 8));
  HOST_TRY (temps.get (&d_res, 32));
  if (out)
    HOST_TRY (temps.get (&d_out, (size_t)out_capacity * sb));
  uint64_t res[4] = { 0, 0, 0, 0 };
  for (;;) {
    const size_t tmp_bytes = acm_gpu_grep_tmp_bytes (plan, room.window, room.capacity, n_symbols, n_texts);
    HOST_TRY (temps.get (&d_tmp, tmp_bytes));
    if (const int rc = settle (plan, acm_gpu_grep_device (plan, d_text, n_symbols, d_off, n_texts, flags, room.window, room.capacity, d_hits, d_kept, d_res,
                                                          d_res + 1, d_res + 2, d_out, out_capacity, d_out_off, out ? d_res + 3 : nullptr, d_tmp, tmp_bytes,
                                                          nullptr), true))
      return rc;
    HOST_TRY (hipMemcpy (res, d_res, 32, hipMemcpyDeviceToHost));
    HOST_TRY (temps.release (d_tmp)); /* (the second attempt's is another size) */
    if (res[2] <= room.capacity)
      break;
    if (!tally_room_shrink (plan, &room))
      return ACM_GPU_E_INTERNAL;
  }
  if (res[0] > n_texts)
    return ACM_GPU_E_INTERNAL;
  *n_kept = res[0];
  if (total)
    *total = res[1];
  if (hits && n_texts)
    HOST_TRY (hipMemcpy (hits, d_hits, n_texts * 8, hipMemcpyDeviceToHost));
  if (kept && res[0])
    HOST_TRY (hipMemcpy (kept, d_kept, res[0] * 4, hipMemcpyDeviceToHost));
  uint64_t symbols = 0; /* (also without an output buffer: the last offset) */
  HOST_TRY (hipMemcpy (&symbols, d_out_off + res[0], 8, hipMemcpyDeviceToHost));
  if (out_offsets)
    HOST_TRY (hipMemcpy (out_offsets, d_out_off, (res[0] + 1) * 8, hipMemcpyDeviceToHost));
  if (out_symbols)
    *out_symbols = symbols;
  if (!out)
    return ACM_GPU_OK;
  if (symbols > out_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (symbols)
    HOST_TRY (hipMemcpy (out, d_out, (size_t)symbols * sb, hipMemcpyDeviceToHost));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_grep_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t flags, uint64_t *hits, uint32_t *kept,
                   uint64_t *n_kept, uint64_t *total, void *out, uint64_t out_capacity, uint64_t *out_offsets, uint64_t *out_symbols) {
  if (!plan || !n_kept || flags > ACM_GREP_INVERT || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  const uint64_t n_symbols = offsets[n_texts];
  HIP_TRY (hipSetDevice (plan->device));
  DeviceTemps temps;
  void *d_text = nullptr;
  uint64_t *d_off = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  return grep_resident (plan, temps, d_text, n_symbols, d_off, n_texts, flags, hits, kept, n_kept, total, out, out_capacity, out_offsets, out_symbols);
}

/* ------------------------------------------------------------------ a buffer cut into texts (include/acm_gpu.h, dev_split.h)
 * Count per tile, prefix sum over the tiles, write.  The plan gives its device, its caller symbol
 * size and its grid cap, nothing else. */
namespace {
/* what split_carve derives beside K's pointers: the tile counts and their sums as the sum takes them */
struct SplitRoom {
  long long *count = nullptr, *begin = nullptr;
  CubRoom cub;
};

/* the scratch is laid out for the most words a text of this size can touch (15 bytes off the grid);
 * n_words and n_tiles are those of the text's own address mod 16, `mis` */
SplitRoom
split_carve (Carve &c, uint64_t n_symbols, uint32_t sb, uint32_t mis, SplitK &K) {
  SplitRoom R;
  /* ACM_GPU_SPLIT_TILE=<bytes of text>: the passes' tile, a multiple of 16 (tests) */
  K.tile_words = tunable ("ACM_GPU_SPLIT_TILE", SPLIT_TILE_DEFAULT, SPLIT_TILE_MIN, SPLIT_TILE_MAX, Tune::Mult16) / 16;
  K.n_words = (n_symbols * sb + mis + 15) / 16;
  K.n_tiles = (K.n_words + K.tile_words - 1) / K.tile_words;
  const uint64_t most_tiles = ((n_symbols * sb + 30) / 16 + K.tile_words - 1) / K.tile_words;
  R.count = c.take<long long> (most_tiles + 1);
  R.begin = c.take<long long> (most_tiles + 1);
  R.cub = cub_room (c, 0, most_tiles + 1);
  K.tile_count = reinterpret_cast<unsigned long long *> (R.count);
  K.tile_begin = reinterpret_cast<const unsigned long long *> (R.begin);
  return R;
}

bool
split_size_ok (const ACMPlan *plan, uint64_t n_symbols) {
  return n_symbols < (1ull << 56) / plan->text_sym_bytes && (n_symbols * plan->text_sym_bytes + 30) / 16 / (SPLIT_TILE_MIN / 16) + 2 < (1ull << 31);
}

template <int SB>
int
split_launch (const ACMPlan *plan, const SplitRoom &L, const SplitK &K, hipStream_t st) {
  HIP_TRY (launch (split_count_kernel<SB>, capped_grid (plan, K.n_tiles + 1), dim3 (SPLIT_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, L.count, L.begin, K.n_tiles + 1, st));
  HIP_TRY (launch (split_write_kernel<SB>, K.offsets ? capped_grid (plan, K.n_tiles) : dim3 (1), dim3 (SPLIT_THREADS), 0, st, K));
  return ACM_GPU_OK;
}
} // namespace

extern "C" size_t
acm_gpu_split_tmp_bytes (const ACMPlan *plan, uint64_t n_symbols) {
  if (!plan || !split_size_ok (plan, n_symbols))
    return 0;
  Carve c;
  SplitK K{};
  split_carve (c, n_symbols, plan->text_sym_bytes, 15, K);
  return c.total ();
}

extern "C" int
acm_gpu_split_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const void *delims, uint32_t n_delims, uint32_t flags, uint64_t *d_offsets,
                      uint64_t capacity, uint64_t *d_n_texts, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_n_texts || !split_args_ok (delims, n_delims, flags) || (n_symbols && !d_text) ||
      (d_offsets && capacity >= (1ull << 31)) || !split_size_ok (plan, n_symbols))
    return ACM_GPU_E_ARG;
  const uint32_t sb = plan->text_sym_bytes;
  const uintptr_t t0 = reinterpret_cast<uintptr_t> (d_text);
  if (t0 % sb)
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  SplitK K{};
  const SplitRoom L = split_carve (carve, n_symbols, sb, (uint32_t)(t0 & 15), K);
  if (n_symbols && (!d_tmp || tmp_bytes < carve.total ()))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  HIP_TRY (hipSetDevice (plan->device));
  if (n_symbols == 0) { /* no symbol: no text, offsets = [0] */
    HIP_TRY (hipMemsetAsync (d_n_texts, 0, 8, st));
    if (d_offsets)
      HIP_TRY (hipMemsetAsync (d_offsets, 0, 8, st));
    return ACM_GPU_OK;
  }
  K.text = static_cast<const unsigned char *> (d_text);
  K.n_symbols = n_symbols;
  for (uint32_t j = 0; j < n_delims; j++) { /* the caller's symbols, bit for bit; below 4 bytes repeated over 32 bits */
    unsigned long long v = 0;
    memcpy (&v, static_cast<const unsigned char *> (delims) + (size_t)j * sb, sb);
    K.delim[j] = sb == 1 ? v * 0x01010101ull : sb == 2 ? v * 0x00010001ull : v;
  }
  K.n_delims = n_delims;
  K.runs = flags == ACM_SPLIT_RUNS;
  K.offsets = reinterpret_cast<unsigned long long *> (d_offsets);
  K.capacity = capacity;
  K.d_n_texts = reinterpret_cast<unsigned long long *> (d_n_texts);
  switch (sb) {
  case 1: return split_launch<1> (plan, L, K, st);
  case 2: return split_launch<2> (plan, L, K, st);
  case 4: return split_launch<4> (plan, L, K, st);
  case 8: return split_launch<8> (plan, L, K, st);
  default: return ACM_GPU_E_ARG;
  }
}

namespace {
/* the count run of a text on the device and its one round trip: *n_texts */
int
split_count_resident (ACMPlan *plan, DeviceTemps &temps, const void *d_text, uint64_t n_symbols, const void *delims, uint32_t n_delims, uint32_t flags,
                      void **d_tmp, size_t *tmp_bytes, uint64_t **d_n, uint64_t *n_texts) {
  *tmp_bytes = acm_gpu_split_tmp_bytes (plan, n_symbols);
  HOST_TRY (temps.get (d_tmp, *tmp_bytes));
  HOST_TRY (temps.get (d_n, 8));
  const int rc = acm_gpu_split_device (plan, d_text, n_symbols, delims, n_delims, flags, nullptr, 0, *d_n, *d_tmp, *tmp_bytes, nullptr);
  if (rc)
    return rc;
  HOST_TRY (hipMemcpy (n_texts, *d_n, 8, hipMemcpyDeviceToHost));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_split_host (ACMPlan *plan, const void *text, uint64_t n_symbols, const void *delims, uint32_t n_delims, uint32_t flags, uint64_t *offsets,
                    uint64_t capacity, uint64_t *n_texts) {
  if (!plan || !n_texts || !split_args_ok (delims, n_delims, flags) || (n_symbols && !text) || !split_size_ok (plan, n_symbols))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_n = nullptr, *d_off = nullptr;
  size_t tmp_bytes = 0;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  int rc = split_count_resident (plan, temps, d_text, n_symbols, delims, n_delims, flags, &d_tmp, &tmp_bytes, &d_n, n_texts);
  if (rc || !offsets)
    return rc;
  if (*n_texts > capacity)
    return ACM_GPU_E_OVERFLOW;
  if (*n_texts >= (1ull << 31))
    return ACM_GPU_E_ARG;
  HOST_TRY (temps.get (&d_off, (*n_texts + 1) * 8));
  rc = acm_gpu_split_device (plan, d_text, n_symbols, delims, n_delims, flags, d_off, *n_texts, d_n, d_tmp, tmp_bytes, nullptr);
  if (rc)
    return rc;
  HOST_TRY (hipMemcpy (offsets, d_off, (*n_texts + 1) * 8, hipMemcpyDeviceToHost));
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_grep_lines_host (ACMPlan *plan, const void *text, uint64_t n_symbols, const void *delims, uint32_t n_delims, uint32_t split_flags,
                         uint32_t grep_flags, uint64_t *n_texts, uint64_t *n_kept, uint64_t *total, void *out, uint64_t out_capacity,
                         uint64_t *out_symbols, uint64_t texts_capacity, uint64_t *offsets, uint64_t *hits, uint32_t *kept, uint64_t *out_offsets) {
  if (!plan || !n_texts || !n_kept || !split_args_ok (delims, n_delims, split_flags) || grep_flags > ACM_GREP_INVERT || (n_symbols && !text) ||
      !split_size_ok (plan, n_symbols))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_n = nullptr, *d_off = nullptr;
  size_t tmp_bytes = 0;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  int rc = split_count_resident (plan, temps, d_text, n_symbols, delims, n_delims, split_flags, &d_tmp, &tmp_bytes, &d_n, n_texts);
  if (rc)
    return rc;
  const uint64_t n = *n_texts;
  if ((offsets || hits || kept || out_offsets) && n > texts_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (n >= (1ull << 31))
    return ACM_GPU_E_ARG;
  HOST_TRY (temps.get (&d_off, (n + 1) * 8));
  rc = acm_gpu_split_device (plan, d_text, n_symbols, delims, n_delims, split_flags, d_off, n, d_n, d_tmp, tmp_bytes, nullptr);
  if (rc)
    return rc;
  if (offsets) /* (the default stream: behind the split) */
    HOST_TRY (hipMemcpy (offsets, d_off, (n + 1) * 8, hipMemcpyDeviceToHost));
  HOST_TRY (temps.release (d_tmp));
  return grep_resident (plan, temps, d_text, n_symbols, d_off, n, grep_flags, hits, kept, n_kept, total, out, out_capacity, out_offsets, out_symbols);
}

/* ------------------------------------------------------------------ per-text keyword counts of a batch (include/acm_gpu.h, dev_tally_batch.h)
 * grep's window walk, every window's records reduced to partial (text, keyword) pairs, then the
 * pairs bucketed by text, merged per row and compacted into the caller's CSR arrays. */
namespace {
/* what tally_batch_carve derives beside K's pointers */
struct TallyBatchRoom {
  uint64_t n_blocks = 0;
  size_t zero_bytes = 0; /* control words, count, pairs per text, row lengths: the head of the scratch, cleared in front of every call */
  uint64_t *d_count = nullptr;
  ACMRecord *rec = nullptr; /* K's, for the passes that write them */
  uint32_t *index = nullptr, *begin = nullptr;
  long long *row_nnz = nullptr, *row_ptr = nullptr;
  CubRoom cub;
};
TallyBatchRoom
tally_batch_carve (Carve &c, const ACMPlan *plan, uint64_t capacity, uint64_t pair_capacity, uint64_t n_symbols, uint64_t n_texts, TbK &K) {
  TallyBatchRoom R;
  R.n_blocks = (n_symbols >> BATCH_BLOCK_LOG2) + 2;
  K.ctl = c.take<TbCtl> (1);
  R.d_count = c.take<uint64_t> (1);
  K.hist = c.take<uint32_t> (n_texts + 1);
  R.row_nnz = c.take<long long> (n_texts + 1);
  R.zero_bytes = c.used;
  K.index = R.index = c.take<uint32_t> (R.n_blocks);
  K.begin = R.begin = c.take<uint32_t> (n_texts + 1);
  R.row_ptr = c.take<long long> (n_texts + 1);
  K.wide = c.take<uint32_t> (n_texts + 1);
  R.cub = cub_room (c, n_texts + 1, n_texts + 1);
  K.mval = K.pkey = c.take<unsigned long long> ((size_t)pair_capacity); /* (the partial pairs are dead behind the scatter: */
  K.mcol = K.pcnt = c.take<uint32_t> ((size_t)pair_capacity);           /* the merged rows take their memory) */
  K.bkw = c.take<uint32_t> ((size_t)pair_capacity);
  K.btext = c.take<uint32_t> ((size_t)pair_capacity);
  K.bval = c.take<unsigned long long> ((size_t)pair_capacity);
  K.whist = c.take<unsigned long long> ((size_t)TB_WIDE_BLOCKS * ((uint64_t)plan->covered_keywords + 1));
  K.rec = R.rec = c.take<ACMRecord> ((size_t)capacity);
  K.row_nnz = reinterpret_cast<unsigned long long *> (R.row_nnz);
  K.row_ptr = reinterpret_cast<const unsigned long long *> (R.row_ptr);
  return R;
}
} // namespace

extern "C" size_t
acm_gpu_tally_batch_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity, uint64_t n_symbols,
                               uint64_t n_texts) {
  (void)window_symbols; /* (what a window's scan needs beside its records belongs to the plan) */
  if (!plan || capacity == 0 || capacity >= (1ull << 31) || pair_capacity == 0 || pair_capacity >= (1ull << 31) || n_texts >= (1ull << 31))
    return 0;
  Carve c;
  TbK K{};
  tally_batch_carve (c, plan, capacity, pair_capacity, n_symbols, n_texts, K);
  return c.total ();
}

extern "C" int
acm_gpu_tally_batch_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint64_t window_symbols,
                            uint64_t capacity, uint64_t pair_capacity, uint64_t *d_row_ptr, uint32_t *d_col, uint64_t *d_val, uint64_t *d_nnz,
                            uint64_t *d_total, uint64_t *d_need, uint64_t *d_need_pairs, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_row_ptr || !d_col || !d_val || !d_nnz || !d_total || !d_need || !d_need_pairs || (n_symbols && !d_text) ||
      !window_ok (window_symbols, capacity) || pair_capacity == 0 || pair_capacity >= (1ull << 31) || n_texts >= (1ull << 31) ||
      !symbols_ok (d_text, n_symbols, plan->text_sym_bytes))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0) /* (an empty matrix) */
    return empty_batch (plan, n_symbols, { d_row_ptr, d_nnz, d_total, d_need, d_need_pairs }, st);
  Carve carve (d_tmp);
  TbK K{};
  const TallyBatchRoom L = tally_batch_carve (carve, plan, capacity, pair_capacity, n_symbols, n_texts, K);
  if (!d_offsets || !d_tmp || tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.capacity = capacity;
  K.n_dev = reinterpret_cast<const unsigned long long *> (L.d_count);
  K.offsets = d_offsets;
  K.n_texts = n_texts;
  K.n_symbols = n_symbols;
  K.n_keywords = plan->covered_keywords;
  /* ACM_GPU_TALLY_BATCH_SLOTS=<a power of two from 8 to 4,096>: the slots of a block's LDS table;
   * ACM_GPU_TALLY_BATCH_ROW=<1 to 2,048>: R, the entries of the widest row merged in LDS (tests, experiments) */
  K.slots = tunable ("ACM_GPU_TALLY_BATCH_SLOTS", TB_SLOTS_DEFAULT, TB_SLOTS_MIN, TB_SLOTS_MAX, Tune::Pow2);
  K.shift = 64;
  for (uint32_t s = K.slots; s > 1; s >>= 1)
    K.shift--;
  K.pair_capacity = pair_capacity;
  K.row = tunable ("ACM_GPU_TALLY_BATCH_ROW", TB_ROW_DEFAULT, 1, TB_ROW_MAX, Tune::Any);
  K.row_p2 = 1;
  while (K.row_p2 < K.row)
    K.row_p2 <<= 1;
  K.d_row_ptr = reinterpret_cast<unsigned long long *> (d_row_ptr);
  K.d_col = d_col;
  K.d_val = reinterpret_cast<unsigned long long *> (d_val);
  K.d_nnz = reinterpret_cast<unsigned long long *> (d_nnz);
  K.d_total = reinterpret_cast<unsigned long long *> (d_total);
  K.d_need = reinterpret_cast<unsigned long long *> (d_need);
  K.d_need_pairs = reinterpret_cast<unsigned long long *> (d_need_pairs);
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  /* 1. the index and the check of offsets[] */
  if (const int bad = batch_index (plan, d_offsets, n_texts, n_symbols, L.index, L.n_blocks, &K.ctl->batch, K.error, st))
    return bad;
  /* 2. every window's records to partial pairs: the grid by the room, two blocks per CU at the most */
  const dim3 pairs_grid = capped_grid (plan, (capacity + TB_THREADS - 1) / TB_THREADS, 2);
  const size_t table_bytes = (size_t)K.slots * 12;
  const int rc = scan_windows (plan, d_text, n_symbols, 0, window_symbols, L.rec, capacity, L.d_count, st, [&] (uint64_t read_begin) -> int {
    K.read_begin = read_begin;
    HIP_TRY (launch (tb_pairs_kernel, pairs_grid, dim3 (TB_THREADS), table_bytes, st, K));
    return ACM_GPU_OK;
  });
  if (rc)
    return rc;
  /* 3. the grids by the room of the pairs */
  const dim3 pair_grid = capped_grid (plan, (pair_capacity + TB_THREADS - 1) / TB_THREADS);
  HIP_TRY (launch (tb_hist_kernel, pair_grid, dim3 (TB_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.hist, L.begin, n_texts + 1, st));
  HIP_TRY (launch (tb_scatter_kernel, pair_grid, dim3 (TB_THREADS), 0, st, K));
  /* 4. */
  HIP_TRY (launch (tb_merge_kernel, capped_grid (plan, (n_texts + TB_TILE - 1) / TB_TILE), dim3 (TB_THREADS), (size_t)K.row_p2 * 16 + ((size_t)K.row_p2 + 1) * 4,
                   st, K));
  HIP_TRY (launch (tb_wide_kernel, dim3 (TB_WIDE_BLOCKS), dim3 (TB_THREADS), 0, st, K));
  /* 5. */
  HIP_TRY (exclusive_sum (L.cub, L.row_nnz, L.row_ptr, n_texts + 1, st));
  HIP_TRY (launch (tb_finish_kernel, capped_grid (plan, (std::max (pair_capacity, n_texts + 1) + TB_THREADS - 1) / TB_THREADS), dim3 (TB_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_tally_batch_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, uint64_t *row_ptr, uint32_t *col, uint64_t *val,
                          uint64_t nnz_capacity, uint64_t *nnz, uint64_t *total) {
  if (!plan || !row_ptr || !nnz || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  const uint64_t n_symbols = offsets[n_texts];
  HIP_TRY (hipSetDevice (plan->device));
  /* the pair room: as many as records of a window, 2^16 at the least, no more than the buffer can have (n x M, to which
   * tally_room has clipped the record room already: the larger of the two before the clip is the larger behind it) */
  RecordRoom room = tally_room (plan, n_symbols);
  uint64_t pair_capacity = std::max<uint64_t> (room.capacity, 1ull << 16);
  const uint64_t most = n_symbols < (1ull << 31) / tally_max_outputs (plan) ? n_symbols * tally_max_outputs (plan) : 1ull << 31;
  if (most < pair_capacity)
    pair_capacity = most ? most : 1;
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_off = nullptr, *d_row_ptr = nullptr, *d_val = nullptr, *d_res = nullptr; /* d_res: nnz, total, need, need_pairs */
  uint32_t *d_col = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  HOST_TRY (temps.get (&d_row_ptr, (n_texts + 1) * 8));
  HOST_TRY (temps.get (&d_res, 32));
  uint64_t res[4] = { 0, 0, 0, 0 };
  bool again_pairs = false;
  for (;;) {
    const size_t tmp_bytes = acm_gpu_tally_batch_tmp_bytes (plan, room.window, room.capacity, pair_capacity, n_symbols, n_texts);
    HOST_TRY (temps.get (&d_tmp, tmp_bytes));
    HOST_TRY (temps.get (&d_col, (size_t)pair_capacity * 4));
    HOST_TRY (temps.get (&d_val, (size_t)pair_capacity * 8));
    if (const int rc = settle (plan, acm_gpu_tally_batch_device (plan, d_text, n_symbols, d_off, n_texts, room.window, room.capacity, pair_capacity,
                                                                 d_row_ptr, d_col, d_val, d_res, d_res + 1, d_res + 2, d_res + 3, d_tmp, tmp_bytes, nullptr),
                               true))
      return rc;
    HOST_TRY (hipMemcpy (res, d_res, 32, hipMemcpyDeviceToHost));
    if (res[2] <= room.capacity && res[3] <= pair_capacity)
      break;
    HOST_TRY (temps.release (d_tmp)); /* (the next attempt's are other sizes) */
    HOST_TRY (temps.release (d_col));
    HOST_TRY (temps.release (d_val));
    if (res[2] > room.capacity) {
      if (!tally_room_shrink (plan, &room))
        return ACM_GPU_E_INTERNAL;
    } else {
      if (again_pairs) /* (the kept records cannot be exceeded: never expected) */
        return ACM_GPU_E_INTERNAL;
      if (res[3] >= (1ull << 31)) /* more partial pairs than one call holds */
        return ACM_GPU_E_NOMEM;
      again_pairs = true;
      pair_capacity = res[3];
    }
  }
  if (res[0] > pair_capacity)
    return ACM_GPU_E_INTERNAL;
  HOST_TRY (hipMemcpy (row_ptr, d_row_ptr, (n_texts + 1) * 8, hipMemcpyDeviceToHost));
  *nnz = res[0];
  if (total)
    *total = res[1];
  if (!col || !val) /* the call only counts */
    return ACM_GPU_OK;
  if (res[0] > nnz_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (res[0]) {
    HOST_TRY (hipMemcpy (col, d_col, res[0] * 4, hipMemcpyDeviceToHost));
    HOST_TRY (hipMemcpy (val, d_val, res[0] * 8, hipMemcpyDeviceToHost));
  }
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ keyword rules per text (include/acm_gpu.h, dev_rules.h)
 * A rule set compiled into an index inverted by keyword, and the passes that evaluate it on a count
 * matrix on the device; acm_gpu_rules_device runs them behind acm_gpu_tally_batch_device. */
struct ACMRules : DeviceSet { /* (the blob: the arrays below, then the two form counters) */
  uint64_t n_rules = 0, n_terms = 0;
  uint32_t n_always = 0, n_postings = 0;
  uint32_t *d_post_ptr = nullptr, *d_base = nullptr, *d_need = nullptr, *d_always = nullptr;
  RulePost *d_post = nullptr;
  unsigned long long *d_forms = nullptr;
};

namespace {
/* what rules_carve derives beside K's pointers */
struct RulesRoom {
  size_t zero_bytes = 0; /* control words and the rows' counts: the head of the scratch, cleared in front of every call */
  long long *cnt = nullptr, *ptr = nullptr; /* K's, as the sum takes them */
  CubRoom cub;
};
/* the part that goes by the texts, and K.wide_p2: what the score passes (below) carve too, in front of their own wide rooms */
RulesRoom
rules_rows_carve (Carve &c, uint32_t n_postings, uint64_t n_texts, RulesK &K) {
  RulesRoom R;
  K.wide_p2 = 1;
  while (K.wide_p2 < n_postings)
    K.wide_p2 <<= 1;
  K.ctl = c.take<RulesCtl> (1);
  R.cnt = c.take<long long> (n_texts + 1);
  R.zero_bytes = c.used;
  R.ptr = c.take<long long> (n_texts + 1);
  K.wide = c.take<uint32_t> (n_texts + 1);
  R.cub = cub_room (c, 0, n_texts + 1);
  K.cnt = reinterpret_cast<unsigned long long *> (R.cnt);
  K.ptr = reinterpret_cast<const unsigned long long *> (R.ptr);
  return R;
}
RulesRoom
rules_carve (Carve &c, const ACMRules *rules, uint64_t n_texts, RulesK &K) {
  const RulesRoom R = rules_rows_carve (c, rules->n_postings, n_texts, K);
  K.wkey = c.take<uint32_t> ((size_t)RULES_WIDE_BLOCKS * K.wide_p2);
  K.wd = c.take<int32_t> ((size_t)RULES_WIDE_BLOCKS * ((size_t)rules->n_postings + 1));
  return R;
}

/* acm_gpu_rules_matrix_tmp_bytes behind its checks */
size_t
rules_bytes (const ACMRules *rules, uint64_t n_texts) {
  Carve c;
  RulesK K{};
  rules_carve (c, rules, n_texts, K);
  return c.total ();
}

/* the matrix calls' own arguments: the set is this plan's device's, the outputs are there */
bool
rules_args_ok (const ACMPlan *plan, const ACMRules *rules, uint64_t n_texts, const uint64_t *d_fired_ptr, const uint32_t *d_fired, uint64_t fired_capacity,
               const uint64_t *d_n_fired) {
  return plan && rules && rules->device == plan->device && n_texts < (1ull << 31) && d_fired_ptr && d_n_fired && (d_fired || fired_capacity == 0);
}

/* the passes of dev_rules.h on a matrix on the device; `tb`: the control words of the tally_batch
 * queued in front, whose stopping stops this call too (nullptr: a caller's matrix) */
int
rules_evaluate (ACMPlan *plan, const ACMRules *rules, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts,
                uint64_t *d_fired_ptr, uint32_t *d_fired, uint64_t fired_capacity, uint64_t *d_n_fired, void *d_tmp, hipStream_t st, const TbCtl *tb,
                uint64_t tb_capacity, uint64_t tb_pair_capacity) {
  Carve carve (d_tmp);
  RulesK K{};
  const RulesRoom L = rules_carve (carve, rules, n_texts, K);
  K.row_ptr = reinterpret_cast<const unsigned long long *> (d_row_ptr);
  K.col = d_col;
  K.val = reinterpret_cast<const unsigned long long *> (d_val);
  K.n_texts = n_texts;
  K.post_ptr = rules->d_post_ptr;
  K.post = rules->d_post;
  K.base = rules->d_base;
  K.need = rules->d_need;
  K.always = rules->d_always;
  K.n_keywords = rules->n_keywords;
  K.n_always = rules->n_always;
  K.n_postings = rules->n_postings;
  K.forms = rules->d_forms;
  /* ACM_GPU_RULES_ITEMS=<1 to 4,096>: the widest text, in items, of the fast form (tests, experiments) */
  K.items = tunable ("ACM_GPU_RULES_ITEMS", RULES_ITEMS_DEFAULT, 1, RULES_ITEMS_MAX, Tune::Any);
  K.items_p2 = 1;
  while (K.items_p2 < K.items)
    K.items_p2 <<= 1;
  K.tb = tb;
  K.tb_capacity = tb_capacity;
  K.tb_pair_capacity = tb_pair_capacity;
  K.d_fired_ptr = reinterpret_cast<unsigned long long *> (d_fired_ptr);
  K.d_n_fired = reinterpret_cast<unsigned long long *> (d_n_fired);
  K.d_fired = d_fired;
  K.fired_capacity = fired_capacity;
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  const dim3 flat_grid = capped_grid (plan, (n_texts + 1 + 255) / 256);
  const dim3 fast_grid = capped_grid (plan, n_texts, RULES_FAST_PER_CU);
  const size_t fast_lds = (size_t)K.items_p2 * 4 + ((size_t)K.items + 1) * 4;
  /* 1. */
  HIP_TRY (launch (rules_check_kernel, flat_grid, dim3 (256), 0, st, K));
  /* 2. */
  HIP_TRY (launch (rules_fast_kernel<false>, fast_grid, dim3 (WAVE), fast_lds, st, K));
  HIP_TRY (launch (rules_wide_kernel<false>, dim3 (RULES_WIDE_BLOCKS), dim3 (RULES_WIDE_THREADS), 0, st, K));
  /* 3. */
  HIP_TRY (exclusive_sum (L.cub, L.cnt, L.ptr, n_texts + 1, st));
  HIP_TRY (launch (rules_finish_kernel, flat_grid, dim3 (256), 0, st, K));
  /* 4. */
  if (d_fired) {
    HIP_TRY (launch (rules_fast_kernel<true>, fast_grid, dim3 (WAVE), fast_lds, st, K));
    HIP_TRY (launch (rules_wide_kernel<true>, dim3 (RULES_WIDE_BLOCKS), dim3 (RULES_WIDE_THREADS), 0, st, K));
  }
  return ACM_GPU_OK;
}

/* where acm_gpu_rules_device and acm_gpu_score_device keep the count matrix and tally_batch's scratch inside their own */
struct RulesCallRoom {
  uint64_t *row_ptr = nullptr, *val = nullptr, *nnz = nullptr;
  uint32_t *col = nullptr;
  unsigned char *tally = nullptr;
  size_t tally_bytes = 0;
  const TbCtl *tb = nullptr; /* tally_batch's control words, where it will put them */
};
RulesCallRoom
rules_call_carve (Carve &c, const ACMPlan *plan, size_t evaluate_bytes, uint64_t capacity, uint64_t pair_capacity, uint64_t n_symbols, uint64_t n_texts) {
  RulesCallRoom R;
  c.used = evaluate_bytes; /* (the evaluation's scratch lies in front, as the matrix call has it) */
  R.row_ptr = c.take<uint64_t> (n_texts + 1);
  R.col = c.take<uint32_t> ((size_t)pair_capacity);
  R.val = c.take<uint64_t> ((size_t)pair_capacity);
  R.nnz = c.take<uint64_t> (1);
  Carve sized;
  TbK T{};
  tally_batch_carve (sized, plan, capacity, pair_capacity, n_symbols, n_texts, T);
  R.tally_bytes = sized.total ();
  R.tally = c.take (R.tally_bytes);
  Carve inner (R.tally);
  tally_batch_carve (inner, plan, capacity, pair_capacity, n_symbols, n_texts, T);
  R.tb = T.ctl;
  return R;
}

/* acm_gpu_tally_batch_device into the matrix of L, then evaluate (), which queues the passes over it; without a text the
 * empty result.  (The arguments that are not checked here are tally_batch's to check.) */
template <typename Evaluate>
int
tally_then_evaluate (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint64_t window_symbols,
                     uint64_t capacity, uint64_t pair_capacity, const RulesCallRoom &L, uint64_t *d_out_ptr, uint64_t *d_n_out, uint64_t *d_total,
                     uint64_t *d_need, uint64_t *d_need_pairs, void *stream, Evaluate evaluate) {
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (const int rc = acm_gpu_tally_batch_device (plan, d_text, n_symbols, d_offsets, n_texts, window_symbols, capacity, pair_capacity, L.row_ptr, L.col,
                                                 L.val, L.nnz, d_total, d_need, d_need_pairs, L.tally, L.tally_bytes, stream))
    return rc;
  if (n_texts == 0) {
    HIP_TRY (hipMemsetAsync (d_out_ptr, 0, 8, st));
    HIP_TRY (hipMemsetAsync (d_n_out, 0, 8, st));
    return ACM_GPU_OK;
  }
  return evaluate ();
}

/* The rooms of a blocking call that runs tally_batch inside: acm_gpu_tally_batch_host's, repeated with what the device
 * reported.  tmp_bytes (window, capacity, pair_capacity) sizes the scratch, call (window, capacity, pair_capacity, d_tmp,
 * tmp_bytes) queues the device call, whose four numbers -- its output count, total, need, need_pairs -- lie at d_res and
 * come back in res[]. */
template <typename TmpBytes, typename Call>
int
with_tally_rooms (ACMPlan *plan, DeviceTemps &temps, uint64_t n_symbols, const uint64_t *d_res, uint64_t res[4], TmpBytes tmp_bytes_of, Call call) {
  RecordRoom room = tally_room (plan, n_symbols);
  uint64_t pair_capacity = std::max<uint64_t> (room.capacity, 1ull << 16);
  const uint64_t most = n_symbols < (1ull << 31) / tally_max_outputs (plan) ? n_symbols * tally_max_outputs (plan) : 1ull << 31;
  if (most < pair_capacity)
    pair_capacity = most ? most : 1;
  void *d_tmp = nullptr;
  bool again_pairs = false;
  for (;;) {
    const size_t tmp_bytes = tmp_bytes_of (room.window, room.capacity, pair_capacity);
    HOST_TRY (temps.get (&d_tmp, tmp_bytes));
    if (const int rc = settle (plan, call (room.window, room.capacity, pair_capacity, d_tmp, tmp_bytes), true))
      return rc;
    HOST_TRY (hipMemcpy (res, d_res, 32, hipMemcpyDeviceToHost));
    if (res[2] <= room.capacity && res[3] <= pair_capacity)
      return ACM_GPU_OK;
    HOST_TRY (temps.release (d_tmp)); /* (the next attempt's is another size) */
    if (res[2] > room.capacity) {
      if (!tally_room_shrink (plan, &room))
        return ACM_GPU_E_INTERNAL;
    } else {
      if (again_pairs) /* (the kept records cannot be exceeded: never expected) */
        return ACM_GPU_E_INTERNAL;
      if (res[3] >= (1ull << 31)) /* more partial pairs than one call holds */
        return ACM_GPU_E_NOMEM;
      again_pairs = true;
      pair_capacity = res[3];
    }
  }
}
} // namespace

extern "C" int
acm_gpu_rules_create (ACMPlan *plan, const ACMRuleTerm *terms, const uint64_t *rule_ptr, const uint32_t *need, uint64_t n_rules, ACMRules **out) {
  if (!plan || !out)
    return ACM_GPU_E_ARG;
  const uint64_t nk = plan->covered_keywords;
  if (acm_rules_check (terms, rule_ptr, need, n_rules, nk) || rule_ptr[n_rules] >= (1ull << 31))
    return ACM_GPU_E_ARG;
  const uint64_t n_terms = rule_ptr[n_rules];
  /* the index: a counting sort of the terms by keyword, rules ascending within a keyword */
  std::vector<uint32_t> post_ptr (nk + 2, 0), base (n_rules ? n_rules : 1, 0), always;
  auto posted = [] (const ACMRuleTerm &q) { return !(q.lo == 0 && q.hi == ACM_RULE_NO_MAX); }; /* (holds at every count: base alone) */
  for (uint64_t i = 0; i < n_terms; i++)
    if (posted (terms[i]))
      post_ptr[terms[i].keyword_id + 2]++;
  for (uint64_t k = 2; k < nk + 2; k++)
    post_ptr[k] += post_ptr[k - 1];
  const uint32_t n_postings = post_ptr[nk + 1];
  std::vector<RulePost> post (n_postings ? n_postings : 1);
  for (uint64_t r = 0; r < n_rules; r++) {
    for (uint64_t i = rule_ptr[r]; i < rule_ptr[r + 1]; i++) {
      const ACMRuleTerm &q = terms[i];
      base[r] += q.lo == 0;
      if (posted (q))
        post[post_ptr[q.keyword_id + 1]++] = RulePost{ (uint32_t)r, q.lo, q.hi };
    }
    if (base[r] >= need[r])
      always.push_back ((uint32_t)r);
  } /* (post_ptr[k + 1] has moved on to the end of k's postings: post_ptr[0 .. nk] are the row pointers now) */
  HIP_TRY (hipSetDevice (plan->device));
  ACMRules *R = new (std::nothrow) ACMRules ();
  if (!R)
    return ACM_GPU_E_NOMEM;
  R->device = plan->device;
  R->n_rules = n_rules;
  R->n_terms = n_terms;
  R->n_keywords = (uint32_t)nk;
  R->n_always = (uint32_t)always.size ();
  R->n_postings = n_postings;
  BlobBuilder b;
  const size_t post_ptr_at = b.add (post_ptr.data (), (nk + 1) * 4), post_at = b.add (post.data (), post.size () * sizeof (RulePost)),
               base_at = b.add (base.data (), base.size () * 4), need_at = b.add (need, n_rules * 4, base.size () * 4),
               always_at = b.add (always.data (), always.size () * 4, (always.size () + 1) * 4), forms_at = b.add (nullptr, 0, 16);
  if (const int rc = set_upload (R, b))
    return rc;
  R->d_post_ptr = b.at<uint32_t> (post_ptr_at);
  R->d_post = b.at<RulePost> (post_at);
  R->d_base = b.at<uint32_t> (base_at);
  R->d_need = b.at<uint32_t> (need_at);
  R->d_always = b.at<uint32_t> (always_at);
  R->d_forms = b.at<unsigned long long> (forms_at);
  *out = R;
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_rules_destroy (ACMRules *rules) {
  set_destroy (rules);
}

extern "C" int
acm_gpu_rules_info (const ACMRules *rules, ACMRulesInfo *info) {
  if (!rules || !info)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (rules->device));
  HIP_TRY (hipDeviceSynchronize ());
  unsigned long long forms[2] = { 0, 0 };
  HIP_TRY (hipMemcpy (forms, rules->d_forms, sizeof forms, hipMemcpyDeviceToHost));
  *info = ACMRulesInfo{ rules->n_rules, rules->n_terms, rules->n_always, rules->n_postings, forms[0], forms[1] };
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_rules_matrix_tmp_bytes (const ACMPlan *plan, const ACMRules *rules, uint64_t n_texts) {
  if (!plan || !rules || n_texts >= (1ull << 31))
    return 0;
  return rules_bytes (rules, n_texts);
}

extern "C" int
acm_gpu_rules_matrix_device (ACMPlan *plan, const ACMRules *rules, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val,
                             uint64_t n_texts, uint64_t *d_fired_ptr, uint32_t *d_fired, uint64_t fired_capacity, uint64_t *d_n_fired, void *d_tmp,
                             size_t tmp_bytes, void *stream) {
  if (!rules_args_ok (plan, rules, n_texts, d_fired_ptr, d_fired, fired_capacity, d_n_fired))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0) { /* no text: an empty matrix */
    HIP_TRY (hipMemsetAsync (d_fired_ptr, 0, 8, st));
    HIP_TRY (hipMemsetAsync (d_n_fired, 0, 8, st));
    return ACM_GPU_OK;
  }
  if (!d_row_ptr || !d_tmp || tmp_bytes < rules_bytes (rules, n_texts))
    return ACM_GPU_E_ARG;
  return rules_evaluate (plan, rules, d_row_ptr, d_col, d_val, n_texts, d_fired_ptr, d_fired, fired_capacity, d_n_fired, d_tmp, st, nullptr, 0, 0);
}

extern "C" size_t
acm_gpu_rules_tmp_bytes (const ACMPlan *plan, const ACMRules *rules, uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity,
                         uint64_t n_symbols, uint64_t n_texts) {
  if (!rules || !acm_gpu_tally_batch_tmp_bytes (plan, window_symbols, capacity, pair_capacity, n_symbols, n_texts))
    return 0;
  Carve c;
  rules_call_carve (c, plan, rules_bytes (rules, n_texts), capacity, pair_capacity, n_symbols, n_texts);
  return c.total ();
}

extern "C" int
acm_gpu_rules_device (ACMPlan *plan, const ACMRules *rules, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts,
                      uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity, uint64_t *d_fired_ptr, uint32_t *d_fired,
                      uint64_t fired_capacity, uint64_t *d_n_fired, uint64_t *d_total, uint64_t *d_need, uint64_t *d_need_pairs, void *d_tmp,
                      size_t tmp_bytes, void *stream) {
  if (!rules_args_ok (plan, rules, n_texts, d_fired_ptr, d_fired, fired_capacity, d_n_fired) || !d_tmp || capacity == 0 || capacity >= (1ull << 31) ||
      pair_capacity == 0 || pair_capacity >= (1ull << 31))
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  const RulesCallRoom L = rules_call_carve (carve, plan, rules_bytes (rules, n_texts), capacity, pair_capacity, n_symbols, n_texts);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  return tally_then_evaluate (plan, d_text, n_symbols, d_offsets, n_texts, window_symbols, capacity, pair_capacity, L, d_fired_ptr, d_n_fired, d_total,
                              d_need, d_need_pairs, stream, [&] {
                                return rules_evaluate (plan, rules, L.row_ptr, L.col, L.val, n_texts, d_fired_ptr, d_fired, fired_capacity, d_n_fired, d_tmp,
                                                       static_cast<hipStream_t> (stream), L.tb, capacity, pair_capacity);
                              });
}

extern "C" int
acm_gpu_rules_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, const ACMRuleTerm *terms, const uint64_t *rule_ptr,
                    const uint32_t *need, uint64_t n_rules, uint64_t *fired_ptr, uint32_t *fired, uint64_t fired_capacity, uint64_t *n_fired,
                    uint64_t *total) {
  if (!plan || !fired_ptr || !n_fired || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  ACMRules *made = nullptr;
  if (const int rc = acm_gpu_rules_create (plan, terms, rule_ptr, need, n_rules, &made))
    return rc;
  std::unique_ptr<ACMRules, void (*) (ACMRules *)> rules (made, acm_gpu_rules_destroy);
  const uint64_t n_symbols = offsets[n_texts];
  DeviceTemps temps;
  void *d_text = nullptr;
  uint64_t *d_off = nullptr, *d_fired_ptr = nullptr, *d_res = nullptr; /* d_res: n_fired, total, need, need_pairs */
  uint32_t *d_fired = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  HOST_TRY (temps.get (&d_fired_ptr, (n_texts + 1) * 8));
  HOST_TRY (temps.get (&d_res, 32));
  if (fired && fired_capacity)
    HOST_TRY (temps.get (&d_fired, (size_t)fired_capacity * 4));
  const uint64_t d_capacity = d_fired ? fired_capacity : 0;
  uint64_t res[4] = { 0, 0, 0, 0 };
  if (const int rc = with_tally_rooms (
        plan, temps, n_symbols, d_res, res,
        [&] (uint64_t window, uint64_t capacity, uint64_t pairs) {
          return acm_gpu_rules_tmp_bytes (plan, rules.get (), window, capacity, pairs, n_symbols, n_texts);
        },
        [&] (uint64_t window, uint64_t capacity, uint64_t pairs, void *d_tmp, size_t tmp_bytes) {
          return acm_gpu_rules_device (plan, rules.get (), d_text, n_symbols, d_off, n_texts, window, capacity, pairs, d_fired_ptr, d_fired, d_capacity,
                                       d_res, d_res + 1, d_res + 2, d_res + 3, d_tmp, tmp_bytes, nullptr);
        }))
    return rc;
  HOST_TRY (hipMemcpy (fired_ptr, d_fired_ptr, (n_texts + 1) * 8, hipMemcpyDeviceToHost));
  *n_fired = res[0];
  if (total)
    *total = res[1];
  if (!fired) /* the call only counts */
    return ACM_GPU_OK;
  if (res[0] > fired_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (res[0])
    HOST_TRY (hipMemcpy (fired, d_fired, res[0] * 4, hipMemcpyDeviceToHost));
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ weighted scores per text (include/acm_score.h, dev_score.h)
 * A model compiled into an index inverted by keyword, the passes that evaluate it on a count matrix on
 * the device and the passes that rank a kept matrix by class; acm_gpu_score_device runs both behind
 * acm_gpu_tally_batch_device. */
struct ACMScore : DeviceSet { /* (the blob: the arrays below, then the two form counters) */
  uint64_t n_classes = 0, n_terms = 0;
  uint32_t n_always = 0, n_postings = 0;
  uint32_t *d_post_ptr = nullptr, *d_always = nullptr;
  ScorePost *d_post = nullptr;
  long long *d_bias = nullptr, *d_threshold = nullptr;
  unsigned long long *d_forms = nullptr;
};

namespace {
RulesRoom
score_carve (Carve &c, const ACMScore *score, uint64_t n_texts, ScoreK &K) {
  const RulesRoom R = rules_rows_carve (c, score->n_postings, n_texts, K.R);
  K.wkey = c.take<unsigned long long> ((size_t)SCORE_WIDE_BLOCKS * K.R.wide_p2);
  K.wval = c.take<unsigned long long> ((size_t)SCORE_WIDE_BLOCKS * ((size_t)score->n_postings + 1));
  return R;
}

/* acm_gpu_score_matrix_tmp_bytes behind its checks */
size_t
score_bytes (const ACMScore *score, uint64_t n_texts) {
  Carve c;
  ScoreK K{};
  score_carve (c, score, n_texts, K);
  return c.total ();
}

/* the matrix calls' own arguments: the model is this plan's device's, the outputs are there */
bool
score_args_ok (const ACMPlan *plan, const ACMScore *score, uint64_t n_texts, const uint64_t *d_kept_ptr, const uint32_t *d_kept_class,
               const int64_t *d_kept_score, uint64_t kept_capacity, const uint64_t *d_n_kept) {
  return plan && score && score->device == plan->device && n_texts < (1ull << 31) && d_kept_ptr && d_n_kept &&
         ((d_kept_class && d_kept_score) || kept_capacity == 0);
}

/* the evaluation passes of dev_score.h on a matrix on the device; `tb` as rules_evaluate has it.  *gate receives the RulesK
 * whose stop tests a top pass behind this call asks. */
int
score_evaluate (ACMPlan *plan, const ACMScore *score, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts,
                uint64_t *d_kept_ptr, uint32_t *d_kept_class, int64_t *d_kept_score, uint64_t kept_capacity, uint64_t *d_n_kept, uint32_t *d_best,
                void *d_tmp, hipStream_t st, const TbCtl *tb, uint64_t tb_capacity, uint64_t tb_pair_capacity, RulesK *gate) {
  Carve carve (d_tmp);
  ScoreK K{};
  const RulesRoom L = score_carve (carve, score, n_texts, K);
  RulesK &R = K.R;
  R.row_ptr = reinterpret_cast<const unsigned long long *> (d_row_ptr);
  R.col = d_col;
  R.val = reinterpret_cast<const unsigned long long *> (d_val);
  R.n_texts = n_texts;
  R.post_ptr = score->d_post_ptr;
  R.always = score->d_always;
  R.n_keywords = score->n_keywords;
  R.n_always = score->n_always;
  R.n_postings = score->n_postings;
  R.forms = score->d_forms;
  /* ACM_GPU_SCORE_ITEMS=<1 to 4,096>: the widest text, in items, of the fast form (tests, experiments) */
  R.items = tunable ("ACM_GPU_SCORE_ITEMS", SCORE_ITEMS_DEFAULT, 1, SCORE_ITEMS_MAX, Tune::Any);
  R.items_p2 = 1;
  while (R.items_p2 < R.items)
    R.items_p2 <<= 1;
  R.tb = tb;
  R.tb_capacity = tb_capacity;
  R.tb_pair_capacity = tb_pair_capacity;
  R.d_fired_ptr = reinterpret_cast<unsigned long long *> (d_kept_ptr);
  R.d_n_fired = reinterpret_cast<unsigned long long *> (d_n_kept);
  R.d_fired = d_kept_class;
  R.fired_capacity = kept_capacity;
  R.error = error_word (plan);
  K.post = score->d_post;
  K.bias = score->d_bias;
  K.threshold = score->d_threshold;
  K.d_kept_score = reinterpret_cast<long long *> (d_kept_score);
  K.d_best = d_best;
  if (gate)
    *gate = R;
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  const dim3 flat_grid = capped_grid (plan, (n_texts + 1 + 255) / 256);
  const size_t fast_lds = ((size_t)R.items_p2 + R.items) * 8;
  /* one-wave blocks a CU: eight at the default room, more at a smaller one and fewer at a larger one by the LDS they take,
   * sixteen (dev_rules.h's number) at the most: 128 KiB of a CU's 160 at every room */
  const uint32_t fast_per_cu =
    (uint32_t)std::min<size_t> (RULES_FAST_PER_CU, std::max<size_t> (1, (size_t)SCORE_FAST_PER_CU * SCORE_ITEMS_DEFAULT * SCORE_ITEM_BYTES / fast_lds));
  const dim3 fast_grid = capped_grid (plan, n_texts, fast_per_cu);
  if (fast_lds + 64 > 64 * 1024) { /* (a room near the largest only: beyond what a kernel may take unasked) */
    HIP_TRY (hipFuncSetAttribute (reinterpret_cast<const void *> (&score_fast_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast_lds));
    HIP_TRY (hipFuncSetAttribute (reinterpret_cast<const void *> (&score_fast_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast_lds));
  }
  /* 1. */
  HIP_TRY (launch (rules_check_kernel, flat_grid, dim3 (256), 0, st, R));
  /* 2. */
  HIP_TRY (launch (score_fast_kernel<false>, fast_grid, dim3 (WAVE), fast_lds, st, K));
  HIP_TRY (launch (score_wide_kernel<false>, dim3 (SCORE_WIDE_BLOCKS), dim3 (SCORE_WIDE_THREADS), 0, st, K));
  /* 3. */
  HIP_TRY (exclusive_sum (L.cub, L.cnt, L.ptr, n_texts + 1, st));
  HIP_TRY (launch (rules_finish_kernel, flat_grid, dim3 (256), 0, st, R));
  /* 4. */
  if (d_kept_class) {
    HIP_TRY (launch (score_fast_kernel<true>, fast_grid, dim3 (WAVE), fast_lds, st, K));
    HIP_TRY (launch (score_wide_kernel<true>, dim3 (SCORE_WIDE_BLOCKS), dim3 (SCORE_WIDE_THREADS), 0, st, K));
  }
  return ACM_GPU_OK;
}

/* what score_top_carve derives beside T's pointers */
struct ScoreTopRoom {
  size_t zero_bytes = 0; /* the gate's control words, the histogram and the cursors: the head of the scratch, cleared in front of every call */
  RulesCtl *ctl = nullptr;
  long long *hist = nullptr, *col_ptr = nullptr; /* T's, as the sum takes them */
  CubRoom cub;
};
ScoreTopRoom
score_top_carve (Carve &c, uint64_t kept_capacity, uint64_t n_classes, ScoreTopK &T) {
  ScoreTopRoom R;
  R.ctl = c.take<RulesCtl> (1);
  R.hist = c.take<long long> (n_classes + 1);
  T.cursor = c.take<unsigned long long> (n_classes + 1);
  R.zero_bytes = c.used;
  R.col_ptr = c.take<long long> (n_classes + 1);
  R.cub = cub_room (c, 0, n_classes + 1);
  T.keys = c.take<ulonglong2> ((size_t)kept_capacity + 1);
  T.hist = reinterpret_cast<unsigned long long *> (R.hist);
  T.col_ptr = reinterpret_cast<const unsigned long long *> (R.col_ptr);
  return R;
}

size_t
score_top_bytes (uint64_t kept_capacity, uint64_t n_classes) {
  Carve c;
  ScoreTopK T{};
  score_top_carve (c, kept_capacity, n_classes, T);
  return c.total ();
}

bool
score_top_args_ok (const ACMPlan *plan, uint64_t kept_capacity, uint64_t n_texts, uint64_t n_classes, uint32_t k) {
  return plan && kept_capacity < (1ull << 31) && n_texts < (1ull << 31) && n_classes < (1ull << 31) && k <= SCORE_TOP_MAX;
}

/* the top passes of dev_score.h over a kept matrix on the device, scratch at d_tmp.  gate: the RulesK of the evaluation
 * queued in front, whose stopping stops these passes too (nullptr: a caller's matrix, whose d_kept_ptr is checked first) */
int
score_top_passes (ACMPlan *plan, const uint64_t *d_kept_ptr, const uint32_t *d_kept_class, const int64_t *d_kept_score, uint64_t kept_capacity,
                  uint64_t n_texts, uint64_t n_classes, uint32_t k, uint64_t *d_class_hits, uint32_t *d_top_n, uint32_t *d_top_text,
                  int64_t *d_top_score, void *d_tmp, hipStream_t st, const RulesK *gate) {
  Carve carve (d_tmp);
  ScoreTopK T{};
  const ScoreTopRoom L = score_top_carve (carve, kept_capacity, n_classes, T);
  T.kept_ptr = reinterpret_cast<const unsigned long long *> (d_kept_ptr);
  T.kept_class = d_kept_class;
  T.kept_score = reinterpret_cast<const long long *> (d_kept_score);
  T.n_texts = n_texts;
  T.kept_capacity = kept_capacity;
  T.n_classes = (uint32_t)n_classes;
  T.k = k;
  T.d_class_hits = reinterpret_cast<unsigned long long *> (d_class_hits);
  T.d_top_n = d_top_n;
  T.d_top_text = d_top_text;
  T.d_top_score = reinterpret_cast<long long *> (d_top_score);
  T.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  if (gate)
    T.G = *gate;
  else {
    T.G.row_ptr = T.kept_ptr;
    T.G.n_texts = n_texts;
    T.G.ctl = L.ctl;
    T.G.error = T.error;
    HIP_TRY (launch (rules_check_kernel, capped_grid (plan, (n_texts + 1 + 255) / 256), dim3 (256), 0, st, T.G));
  }
  const dim3 entry_grid = capped_grid (plan, (kept_capacity + 255) / 256);
  /* 1. */
  HIP_TRY (launch (score_top_hist_kernel, entry_grid, dim3 (256), 0, st, T));
  /* 2. */
  HIP_TRY (exclusive_sum (L.cub, L.hist, L.col_ptr, n_classes + 1, st));
  /* 3. */
  HIP_TRY (launch (score_top_scatter_kernel, entry_grid, dim3 (256), 0, st, T));
  /* 4. */
  /* ACM_GPU_SCORE_TOP_BLOCKS=<1 to 65,536>: the most blocks of the select pass, so that tests make it stride over few classes */
  const uint32_t most_blocks = tunable ("ACM_GPU_SCORE_TOP_BLOCKS", 65536, 1, 65536, Tune::Any);
  HIP_TRY (launch (score_top_select_kernel, capped_grid (plan, std::min<uint64_t> (n_classes, most_blocks), 4), dim3 (SCORE_TOP_THREADS), 0, st, T));
  return ACM_GPU_OK;
}

/* whether a call that evaluates is to rank as well */
bool
score_wants_top (uint32_t k, const uint64_t *class_hits, const uint32_t *top_n, const uint32_t *top_text, const int64_t *top_score) {
  return k > 0 && class_hits && top_n && top_text && top_score;
}
} // namespace

extern "C" int
acm_gpu_score_create (ACMPlan *plan, const ACMScoreTerm *terms, const uint64_t *class_ptr, const int64_t *bias, const int64_t *threshold,
                      uint64_t n_classes, ACMScore **out) {
  if (!plan || !out)
    return ACM_GPU_E_ARG;
  const uint64_t nk = plan->covered_keywords;
  if (acm_score_check (terms, class_ptr, bias, threshold, n_classes, nk))
    return ACM_GPU_E_ARG;
  const uint64_t n_terms = class_ptr[n_classes];
  /* the index: a counting sort of the terms by keyword, classes ascending within a keyword */
  std::vector<uint32_t> post_ptr (nk + 2, 0), always;
  for (uint64_t i = 0; i < n_terms; i++)
    if (terms[i].weight != 0) /* (a weight of 0 adds nothing at any count) */
      post_ptr[terms[i].keyword_id + 2]++;
  for (uint64_t k = 2; k < nk + 2; k++)
    post_ptr[k] += post_ptr[k - 1];
  const uint32_t n_postings = post_ptr[nk + 1];
  std::vector<ScorePost> post (n_postings ? n_postings : 1);
  for (uint64_t c = 0; c < n_classes; c++) {
    for (uint64_t i = class_ptr[c]; i < class_ptr[c + 1]; i++) {
      const ACMScoreTerm &q = terms[i];
      if (q.weight != 0)
        post[post_ptr[q.keyword_id + 1]++] = ScorePost{ (uint32_t)c, q.weight, q.cap };
    }
    if (bias[c] >= threshold[c])
      always.push_back ((uint32_t)c);
  } /* (post_ptr[k + 1] has moved on to the end of k's postings: post_ptr[0 .. nk] are the row pointers now) */
  HIP_TRY (hipSetDevice (plan->device));
  ACMScore *S = new (std::nothrow) ACMScore ();
  if (!S)
    return ACM_GPU_E_NOMEM;
  S->device = plan->device;
  S->n_classes = n_classes;
  S->n_terms = n_terms;
  S->n_keywords = (uint32_t)nk;
  S->n_always = (uint32_t)always.size ();
  S->n_postings = n_postings;
  const size_t classes_bytes = (n_classes ? n_classes : 1) * 8;
  BlobBuilder b;
  const size_t post_ptr_at = b.add (post_ptr.data (), (nk + 1) * 4), post_at = b.add (post.data (), post.size () * sizeof (ScorePost)),
               bias_at = b.add (bias, n_classes * 8, classes_bytes), threshold_at = b.add (threshold, n_classes * 8, classes_bytes),
               always_at = b.add (always.data (), always.size () * 4, (always.size () + 1) * 4), forms_at = b.add (nullptr, 0, 16);
  if (const int rc = set_upload (S, b))
    return rc;
  S->d_post_ptr = b.at<uint32_t> (post_ptr_at);
  S->d_post = b.at<ScorePost> (post_at);
  S->d_bias = b.at<long long> (bias_at);
  S->d_threshold = b.at<long long> (threshold_at);
  S->d_always = b.at<uint32_t> (always_at);
  S->d_forms = b.at<unsigned long long> (forms_at);
  *out = S;
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_score_destroy (ACMScore *score) {
  set_destroy (score);
}

extern "C" int
acm_gpu_score_info (const ACMScore *score, ACMScoreInfo *info) {
  if (!score || !info)
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (score->device));
  HIP_TRY (hipDeviceSynchronize ());
  unsigned long long forms[2] = { 0, 0 };
  HIP_TRY (hipMemcpy (forms, score->d_forms, sizeof forms, hipMemcpyDeviceToHost));
  *info = ACMScoreInfo{ score->n_classes, score->n_terms, score->n_postings, score->n_always, forms[0], forms[1] };
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_score_matrix_tmp_bytes (const ACMPlan *plan, const ACMScore *score, uint64_t n_texts) {
  if (!plan || !score || n_texts >= (1ull << 31))
    return 0;
  return score_bytes (score, n_texts);
}

extern "C" int
acm_gpu_score_matrix_device (ACMPlan *plan, const ACMScore *score, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val,
                             uint64_t n_texts, uint64_t *d_kept_ptr, uint32_t *d_kept_class, int64_t *d_kept_score, uint64_t kept_capacity,
                             uint64_t *d_n_kept, uint32_t *d_best, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!score_args_ok (plan, score, n_texts, d_kept_ptr, d_kept_class, d_kept_score, kept_capacity, d_n_kept))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0) { /* no text: an empty matrix */
    HIP_TRY (hipMemsetAsync (d_kept_ptr, 0, 8, st));
    HIP_TRY (hipMemsetAsync (d_n_kept, 0, 8, st));
    return ACM_GPU_OK;
  }
  if (!d_row_ptr || !d_tmp || tmp_bytes < score_bytes (score, n_texts))
    return ACM_GPU_E_ARG;
  return score_evaluate (plan, score, d_row_ptr, d_col, d_val, n_texts, d_kept_ptr, d_kept_class, d_kept_score, kept_capacity, d_n_kept, d_best, d_tmp,
                         st, nullptr, 0, 0, nullptr);
}

extern "C" size_t
acm_gpu_score_top_tmp_bytes (const ACMPlan *plan, uint64_t kept_capacity, uint64_t n_classes) {
  if (!score_top_args_ok (plan, kept_capacity, 0, n_classes, 0))
    return 0;
  return score_top_bytes (kept_capacity, n_classes);
}

extern "C" int
acm_gpu_score_top_device (ACMPlan *plan, const uint64_t *d_kept_ptr, const uint32_t *d_kept_class, const int64_t *d_kept_score, uint64_t kept_capacity,
                          uint64_t n_texts, uint64_t n_classes, uint32_t k, uint64_t *d_class_hits, uint32_t *d_top_n, uint32_t *d_top_text,
                          int64_t *d_top_score, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!score_top_args_ok (plan, kept_capacity, n_texts, n_classes, k) || !d_kept_ptr || (kept_capacity && (!d_kept_class || !d_kept_score)) ||
      (n_classes && (!d_class_hits || !d_top_n || (k && (!d_top_text || !d_top_score)))) || !d_tmp ||
      tmp_bytes < score_top_bytes (kept_capacity, n_classes))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  return score_top_passes (plan, d_kept_ptr, d_kept_class, d_kept_score, kept_capacity, n_texts, n_classes, k, d_class_hits, d_top_n, d_top_text,
                           d_top_score, d_tmp, static_cast<hipStream_t> (stream), nullptr);
}

extern "C" size_t
acm_gpu_score_tmp_bytes (const ACMPlan *plan, const ACMScore *score, uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity,
                         uint64_t n_symbols, uint64_t n_texts, uint64_t kept_capacity, uint32_t k) {
  if (!score || !score_top_args_ok (plan, kept_capacity, n_texts, score->n_classes, k) ||
      !acm_gpu_tally_batch_tmp_bytes (plan, window_symbols, capacity, pair_capacity, n_symbols, n_texts))
    return 0;
  Carve c;
  rules_call_carve (c, plan, score_bytes (score, n_texts), capacity, pair_capacity, n_symbols, n_texts);
  if (k)
    c.take (score_top_bytes (kept_capacity, score->n_classes));
  return c.total ();
}

extern "C" int
acm_gpu_score_device (ACMPlan *plan, const ACMScore *score, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts,
                      uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity, uint64_t *d_kept_ptr, uint32_t *d_kept_class,
                      int64_t *d_kept_score, uint64_t kept_capacity, uint64_t *d_n_kept, uint32_t *d_best, uint32_t k, uint64_t *d_class_hits,
                      uint32_t *d_top_n, uint32_t *d_top_text, int64_t *d_top_score, uint64_t *d_total, uint64_t *d_need, uint64_t *d_need_pairs,
                      void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!score_args_ok (plan, score, n_texts, d_kept_ptr, d_kept_class, d_kept_score, kept_capacity, d_n_kept) ||
      !score_top_args_ok (plan, kept_capacity, n_texts, score->n_classes, k) || !d_tmp || capacity == 0 || capacity >= (1ull << 31) ||
      pair_capacity == 0 || pair_capacity >= (1ull << 31))
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  const RulesCallRoom L = rules_call_carve (carve, plan, score_bytes (score, n_texts), capacity, pair_capacity, n_symbols, n_texts);
  void *d_top_tmp = k ? carve.take (score_top_bytes (kept_capacity, score->n_classes)) : nullptr;
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  const bool top = score_wants_top (k, d_class_hits, d_top_n, d_top_text, d_top_score) && d_kept_class;
  return tally_then_evaluate (
    plan, d_text, n_symbols, d_offsets, n_texts, window_symbols, capacity, pair_capacity, L, d_kept_ptr, d_n_kept, d_total, d_need, d_need_pairs, stream, [&] {
      hipStream_t st = static_cast<hipStream_t> (stream);
      RulesK gate{};
      if (const int rc = score_evaluate (plan, score, L.row_ptr, L.col, L.val, n_texts, d_kept_ptr, d_kept_class, d_kept_score, kept_capacity, d_n_kept,
                                         d_best, d_tmp, st, L.tb, capacity, pair_capacity, &gate))
        return rc;
      return top ? score_top_passes (plan, d_kept_ptr, d_kept_class, d_kept_score, kept_capacity, n_texts, score->n_classes, k, d_class_hits, d_top_n,
                                     d_top_text, d_top_score, d_top_tmp, st, &gate)
                 : (int)ACM_GPU_OK;
    });
}

extern "C" int
acm_gpu_score_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, const ACMScoreTerm *terms, const uint64_t *class_ptr,
                    const int64_t *bias, const int64_t *threshold, uint64_t n_classes, uint64_t *kept_ptr, uint32_t *kept_class, int64_t *kept_score,
                    uint64_t kept_capacity, uint64_t *n_kept, uint32_t *best, uint32_t k, uint64_t *class_hits, uint32_t *top_n, uint32_t *top_text,
                    int64_t *top_score, uint64_t *total) {
  if (!plan || !kept_ptr || !n_kept || k > SCORE_TOP_MAX || kept_capacity >= (1ull << 31) || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  ACMScore *made = nullptr;
  if (const int rc = acm_gpu_score_create (plan, terms, class_ptr, bias, threshold, n_classes, &made))
    return rc;
  std::unique_ptr<ACMScore, void (*) (ACMScore *)> score (made, acm_gpu_score_destroy);
  const uint64_t n_symbols = offsets[n_texts];
  const bool fills = kept_class && kept_score && kept_capacity;
  const bool top = fills && n_classes && score_wants_top (k, class_hits, top_n, top_text, top_score);
  const uint32_t d_k = top ? k : 0;
  DeviceTemps temps;
  void *d_text = nullptr;
  uint64_t *d_off = nullptr, *d_kept_ptr = nullptr, *d_res = nullptr, *d_hits = nullptr; /* d_res: n_kept, total, need, need_pairs */
  uint32_t *d_kept_class = nullptr, *d_best = nullptr, *d_top_n = nullptr, *d_top_text = nullptr;
  int64_t *d_kept_score = nullptr, *d_top_score = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  HOST_TRY (temps.get (&d_kept_ptr, (n_texts + 1) * 8));
  HOST_TRY (temps.get (&d_res, 32));
  if (fills) {
    HOST_TRY (temps.get (&d_kept_class, (size_t)kept_capacity * 4));
    HOST_TRY (temps.get (&d_kept_score, (size_t)kept_capacity * 8));
    if (best && n_texts)
      HOST_TRY (temps.get (&d_best, (size_t)n_texts * 4));
  }
  if (top) {
    HOST_TRY (temps.get (&d_hits, (size_t)n_classes * 8));
    HOST_TRY (temps.get (&d_top_n, (size_t)n_classes * 4));
    HOST_TRY (temps.get (&d_top_text, (size_t)n_classes * k * 4));
    HOST_TRY (temps.get (&d_top_score, (size_t)n_classes * k * 8));
  }
  const uint64_t d_capacity = fills ? kept_capacity : 0;
  uint64_t res[4] = { 0, 0, 0, 0 };
  if (const int rc = with_tally_rooms (
        plan, temps, n_symbols, d_res, res,
        [&] (uint64_t window, uint64_t capacity, uint64_t pairs) {
          return acm_gpu_score_tmp_bytes (plan, score.get (), window, capacity, pairs, n_symbols, n_texts, d_capacity, d_k);
        },
        [&] (uint64_t window, uint64_t capacity, uint64_t pairs, void *d_tmp, size_t tmp_bytes) {
          return acm_gpu_score_device (plan, score.get (), d_text, n_symbols, d_off, n_texts, window, capacity, pairs, d_kept_ptr, d_kept_class,
                                       d_kept_score, d_capacity, d_res, d_best, d_k, d_hits, d_top_n, d_top_text, d_top_score, d_res + 1, d_res + 2,
                                       d_res + 3, d_tmp, tmp_bytes, nullptr);
        }))
    return rc;
  HOST_TRY (hipMemcpy (kept_ptr, d_kept_ptr, (n_texts + 1) * 8, hipMemcpyDeviceToHost));
  *n_kept = res[0];
  if (total)
    *total = res[1];
  if (!kept_class || !kept_score) /* the call only counts */
    return ACM_GPU_OK;
  if (res[0] > kept_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (res[0]) {
    HOST_TRY (hipMemcpy (kept_class, d_kept_class, res[0] * 4, hipMemcpyDeviceToHost));
    HOST_TRY (hipMemcpy (kept_score, d_kept_score, res[0] * 8, hipMemcpyDeviceToHost));
  }
  if (best && n_texts) {
    if (d_best)
      HOST_TRY (hipMemcpy (best, d_best, n_texts * 4, hipMemcpyDeviceToHost));
    else /* (no room and nothing kept: every row is empty) */
      std::fill (best, best + n_texts, ACM_SCORE_NONE);
  }
  if (top) {
    if (n_texts) {
      HOST_TRY (hipMemcpy (class_hits, d_hits, n_classes * 8, hipMemcpyDeviceToHost));
      HOST_TRY (hipMemcpy (top_n, d_top_n, n_classes * 4, hipMemcpyDeviceToHost));
      HOST_TRY (hipMemcpy (top_text, d_top_text, n_classes * k * 4, hipMemcpyDeviceToHost));
      HOST_TRY (hipMemcpy (top_score, d_top_score, n_classes * k * 8, hipMemcpyDeviceToHost));
    } else /* (no text: the device call ends behind the tally) */
      return acm_score_top (kept_ptr, kept_class, kept_score, 0, n_classes, k, class_hits, top_n, top_text, top_score);
  } else if (n_classes && score_wants_top (k, class_hits, top_n, top_text, top_score)) /* (nothing kept and no room: every column is empty) */
    return acm_score_top (kept_ptr, kept_class, kept_score, n_texts, n_classes, k, class_hits, top_n, top_text, top_score);
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ the inverted index of a batch (include/acm_index.h, dev_index.h)
 * The passes that transpose a count matrix on the device into the postings of every keyword, and the
 * concatenation of two indexes; acm_gpu_index_device runs the former behind acm_gpu_tally_batch_device. */
namespace {
size_t
index_sort_bytes (uint64_t n) {
  size_t tmp = 0;
  hipcub::DoubleBuffer<unsigned long long> k (nullptr, nullptr), v (nullptr, nullptr);
  (void)hipcub::DeviceRadixSort::SortPairs (nullptr, tmp, k, v, (int)n, 0, 64, nullptr);
  return tmp;
}

/* ACM_GPU_INDEX_LIST=<1 to 4,096>: the longest list of the fast form (tests, experiments) */
uint32_t
index_list () {
  return tunable ("ACM_GPU_INDEX_LIST", INDEX_LIST_DEFAULT, 1, INDEX_LIST_MAX, Tune::Any);
}

/* LDS of index_sort_kernel for lists of up to `longest` entries: the keys, padded to a power of two, and the counts */
size_t
index_sort_lds (uint32_t longest) {
  uint32_t p2 = 1;
  while (p2 < longest)
    p2 <<= 1;
  return ((size_t)p2 + longest) * 8;
}

/* what index_carve derives beside K's pointers */
struct IndexRoom {
  size_t zero_bytes = 0; /* control words and the keywords' counts: the head of the scratch, cleared in front of every call */
  long long *cnt = nullptr, *ptr = nullptr, *wcnt = nullptr, *wbase = nullptr; /* K's, as the sums take them */
  unsigned long long *key[2] = { nullptr, nullptr }, *val[2] = { nullptr, nullptr }; /* the sort room and its second half */
  CubRoom cub;
  void *sort_tmp = nullptr;
  size_t sort_bytes = 0;
};
/* wide: the call has a wide form (n_texts above the fast form's longest list, and a room to fill) */
IndexRoom
index_carve (Carve &c, uint64_t n_keywords, uint64_t post_capacity, bool wide, IndexK &K) {
  IndexRoom R;
  K.G.ctl = c.take<RulesCtl> (1);
  K.ictl = c.take<IndexCtl> (1);
  R.cnt = c.take<long long> (n_keywords + 1);
  R.zero_bytes = c.used;
  R.ptr = c.take<long long> (n_keywords + 1);
  R.cub = cub_room (c, 0, n_keywords + 1);
  K.tier = c.take<uint32_t> (n_keywords);
  if (wide) {
    R.wcnt = c.take<long long> (n_keywords + 1);
    R.wbase = c.take<long long> (n_keywords + 1);
    for (int h = 0; h < 2; h++) {
      R.key[h] = c.take<unsigned long long> ((size_t)post_capacity);
      R.val[h] = c.take<unsigned long long> ((size_t)post_capacity);
    }
    R.sort_bytes = index_sort_bytes (post_capacity);
    R.sort_tmp = c.take (R.sort_bytes + 16);
  }
  K.cnt = reinterpret_cast<unsigned long long *> (R.cnt);
  K.ptr = reinterpret_cast<const unsigned long long *> (R.ptr);
  K.wcnt = reinterpret_cast<unsigned long long *> (R.wcnt);
  K.wbase = reinterpret_cast<const unsigned long long *> (R.wbase);
  K.wkey = R.key[0];
  K.wval = R.val[0];
  return R;
}

bool
index_wide (uint64_t n_texts, uint64_t post_capacity) {
  return post_capacity > 0 && n_texts > index_list ();
}

/* acm_gpu_index_matrix_tmp_bytes behind its checks */
size_t
index_bytes (uint64_t n_texts, uint64_t n_keywords, uint64_t post_capacity) {
  Carve c;
  IndexK K{};
  index_carve (c, n_keywords, post_capacity, index_wide (n_texts, post_capacity), K);
  return c.total ();
}

/* the matrix calls' own arguments */
bool
index_args_ok (const ACMPlan *plan, uint64_t n_texts, uint64_t n_keywords, uint64_t text_base, const uint64_t *d_post_ptr, const uint32_t *d_post_text,
               const uint64_t *d_post_count, uint64_t post_capacity, const uint64_t *d_nnz) {
  return plan && n_texts < (1ull << 31) && n_keywords >= plan->covered_keywords && n_keywords < (1ull << 32) && text_base <= (1ull << 32) &&
         text_base + n_texts <= (1ull << 32) && post_capacity < (1ull << 31) && d_post_ptr && d_nnz &&
         ((d_post_text && d_post_count) || (post_capacity == 0 && !d_post_text && !d_post_count));
}

/* without a text: every list is empty */
int
index_empty (uint64_t n_keywords, uint64_t *d_post_ptr, uint64_t *d_nnz, uint64_t *d_forms, hipStream_t st) {
  HIP_TRY (hipMemsetAsync (d_post_ptr, 0, (n_keywords + 1) * 8, st));
  HIP_TRY (hipMemsetAsync (d_nnz, 0, 8, st));
  if (d_forms)
    HIP_TRY (hipMemsetAsync (d_forms, 0, 16, st));
  return ACM_GPU_OK;
}

/* the passes of dev_index.h on a matrix on the device; `tb` as rules_evaluate has it */
int
index_transpose (ACMPlan *plan, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts, uint64_t n_keywords,
                 uint64_t text_base, uint64_t *d_post_ptr, uint32_t *d_post_text, uint64_t *d_post_count, uint64_t post_capacity, uint64_t *d_nnz,
                 uint64_t *d_forms, void *d_tmp, hipStream_t st, const TbCtl *tb, uint64_t tb_capacity, uint64_t tb_pair_capacity) {
  Carve carve (d_tmp);
  IndexK K{};
  const bool wide = index_wide (n_texts, post_capacity);
  const IndexRoom L = index_carve (carve, n_keywords, post_capacity, wide, K);
  K.G.row_ptr = reinterpret_cast<const unsigned long long *> (d_row_ptr);
  K.G.n_texts = n_texts;
  K.G.tb = tb;
  K.G.tb_capacity = tb_capacity;
  K.G.tb_pair_capacity = tb_pair_capacity;
  K.G.error = error_word (plan);
  K.col = d_col;
  K.val = reinterpret_cast<const unsigned long long *> (d_val);
  K.n_keywords = n_keywords;
  K.text_base = text_base;
  K.post_capacity = post_capacity;
  K.list = index_list ();
  K.d_post_ptr = reinterpret_cast<unsigned long long *> (d_post_ptr);
  K.d_post_text = d_post_text;
  K.d_post_count = reinterpret_cast<unsigned long long *> (d_post_count);
  K.d_nnz = reinterpret_cast<unsigned long long *> (d_nnz);
  K.d_forms = reinterpret_cast<unsigned long long *> (d_forms);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  /* the grids of the passes over the matrix's entries: the device alone knows how many there are.  Two blocks a CU count:
   * every block ends with an atomic per LDS counter it used */
  const dim3 entry_grid = capped_grid (plan, ~0ull), hist_grid = capped_grid (plan, ~0ull, 2),
             keyword_grid = capped_grid (plan, (n_keywords + 1 + 255) / 256);
  /* 1. */
  HIP_TRY (launch (rules_check_kernel, capped_grid (plan, (n_texts + 1 + 255) / 256), dim3 (256), 0, st, K.G));
  /* 2. */
  HIP_TRY (launch (index_hist_kernel, hist_grid, dim3 (256), 0, st, K));
  /* 3. */
  HIP_TRY (exclusive_sum (L.cub, L.cnt, L.ptr, n_keywords + 1, st));
  HIP_TRY (launch (index_finish_kernel, keyword_grid, dim3 (256), 0, st, K));
  if (d_post_text) {
    if (wide) {
      HIP_TRY (exclusive_sum (L.cub, L.wcnt, L.wbase, n_keywords + 1, st));
      HIP_TRY (hipMemsetAsync (L.key[0], 0xFF, (size_t)post_capacity * 8, st)); /* the sentinels */
    }
    /* 4. */
    HIP_TRY (launch (index_scatter_kernel, entry_grid, dim3 (256), 0, st, K));
    /* 5. (a block per list of the tier: the host knows no more than that there are at most n_keywords) */
    const uint32_t wave_list = std::min (K.list, INDEX_WAVE_LIST);
    if (wave_list >= 2)
      HIP_TRY (launch (index_sort_kernel<WAVE, 0>, capped_grid (plan, n_keywords, 16), dim3 (WAVE), index_sort_lds (wave_list), st, K, wave_list));
    if (K.list > INDEX_WAVE_LIST) {
      const size_t lds = index_sort_lds (K.list);
      if (lds + 64 > 64 * 1024) /* (the longest list only: beyond what a kernel may take unasked) */
        HIP_TRY (hipFuncSetAttribute (reinterpret_cast<const void *> (&index_sort_kernel<INDEX_SORT_THREADS, 1>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      const uint32_t per_cu = (uint32_t)std::max<size_t> (1, std::min<size_t> (8, (128 * 1024) / lds));
      HIP_TRY (launch (index_sort_kernel<INDEX_SORT_THREADS, 1>, capped_grid (plan, n_keywords, per_cu), dim3 (INDEX_SORT_THREADS), lds, st, K, K.list));
    }
    /* 6. */
    if (wide) {
      int key_bits = INDEX_TEXT_BITS + 1;
      while (key_bits < 63 && (n_keywords >> (key_bits - INDEX_TEXT_BITS)) != 0)
        key_bits++;
      hipcub::DoubleBuffer<unsigned long long> keys (L.key[0], L.key[1]), vals (L.val[0], L.val[1]);
      size_t sort_bytes = L.sort_bytes;
      HIP_TRY (hipcub::DeviceRadixSort::SortPairs (L.sort_tmp, sort_bytes, keys, vals, (int)post_capacity, 0, key_bits, st));
      K.skey = keys.Current ();
      K.sval = vals.Current ();
      HIP_TRY (launch (index_wide_put_kernel, capped_grid (plan, (post_capacity + 255) / 256), dim3 (256), 0, st, K));
    }
  }
  if (d_forms)
    HIP_TRY (launch (index_forms_kernel, dim3 (1), dim3 (WAVE), 0, st, K));
  return ACM_GPU_OK;
}

bool
index_concat_args_ok (const ACMPlan *plan, const uint64_t *d_a_ptr, uint64_t n_keywords_a, const uint64_t *d_b_ptr, uint64_t n_keywords_b,
                      const uint64_t *d_out_ptr, const uint32_t *d_out_text, const uint64_t *d_out_count, uint64_t out_capacity,
                      const uint64_t *d_out_nnz) {
  return plan && d_a_ptr && d_b_ptr && n_keywords_a <= n_keywords_b && n_keywords_b < (1ull << 32) && out_capacity < (1ull << 31) && d_out_ptr &&
         d_out_nnz && ((d_out_text && d_out_count) || (out_capacity == 0 && !d_out_text && !d_out_count));
}
} // namespace

extern "C" size_t
acm_gpu_index_matrix_tmp_bytes (const ACMPlan *plan, uint64_t n_texts, uint64_t n_keywords, uint64_t post_capacity) {
  if (!plan || n_texts >= (1ull << 31) || n_keywords >= (1ull << 32) || post_capacity >= (1ull << 31))
    return 0;
  return index_bytes (n_texts, n_keywords, post_capacity);
}

extern "C" int
acm_gpu_index_matrix_device (ACMPlan *plan, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts, uint64_t n_keywords,
                             uint64_t text_base, uint64_t *d_post_ptr, uint32_t *d_post_text, uint64_t *d_post_count, uint64_t post_capacity,
                             uint64_t *d_nnz, uint64_t *d_forms, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!index_args_ok (plan, n_texts, n_keywords, text_base, d_post_ptr, d_post_text, d_post_count, post_capacity, d_nnz))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0)
    return index_empty (n_keywords, d_post_ptr, d_nnz, d_forms, st);
  if (!d_row_ptr || !d_tmp || tmp_bytes < index_bytes (n_texts, n_keywords, post_capacity))
    return ACM_GPU_E_ARG;
  return index_transpose (plan, d_row_ptr, d_col, d_val, n_texts, n_keywords, text_base, d_post_ptr, d_post_text, d_post_count, post_capacity, d_nnz, d_forms,
                          d_tmp, st, nullptr, 0, 0);
}

extern "C" size_t
acm_gpu_index_concat_tmp_bytes (const ACMPlan *plan, uint64_t n_keywords_b) {
  if (!plan || n_keywords_b >= (1ull << 32))
    return 0;
  Carve c;
  c.take<RulesCtl> (1);
  return c.total ();
}

extern "C" int
acm_gpu_index_concat_device (ACMPlan *plan, const uint64_t *d_a_ptr, const uint32_t *d_a_text, const uint64_t *d_a_count, uint64_t n_keywords_a,
                             const uint64_t *d_b_ptr, const uint32_t *d_b_text, const uint64_t *d_b_count, uint64_t n_keywords_b, uint64_t *d_out_ptr,
                             uint32_t *d_out_text, uint64_t *d_out_count, uint64_t out_capacity, uint64_t *d_out_nnz, void *d_tmp, size_t tmp_bytes,
                             void *stream) {
  if (!index_concat_args_ok (plan, d_a_ptr, n_keywords_a, d_b_ptr, n_keywords_b, d_out_ptr, d_out_text, d_out_count, out_capacity, d_out_nnz) || !d_tmp ||
      tmp_bytes < acm_gpu_index_concat_tmp_bytes (plan, n_keywords_b))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  Carve carve (d_tmp);
  IndexCatK C{};
  C.ctl = carve.take<RulesCtl> (1);
  C.a_ptr = reinterpret_cast<const unsigned long long *> (d_a_ptr);
  C.b_ptr = reinterpret_cast<const unsigned long long *> (d_b_ptr);
  C.a_count = reinterpret_cast<const unsigned long long *> (d_a_count);
  C.b_count = reinterpret_cast<const unsigned long long *> (d_b_count);
  C.a_text = d_a_text;
  C.b_text = d_b_text;
  C.n_a = n_keywords_a;
  C.n_b = n_keywords_b;
  C.out_capacity = out_capacity;
  C.d_out_ptr = reinterpret_cast<unsigned long long *> (d_out_ptr);
  C.d_out_nnz = reinterpret_cast<unsigned long long *> (d_out_nnz);
  C.d_out_count = reinterpret_cast<unsigned long long *> (d_out_count);
  C.d_out_text = d_out_text;
  C.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (C.ctl, 0, sizeof (RulesCtl), st));
  const dim3 keyword_grid = capped_grid (plan, (n_keywords_b + 1 + 255) / 256);
  /* the count pass: the pointer arrays, then (an address is formed from them only now) the boundaries, then out_ptr */
  HIP_TRY (launch (index_concat_check_kernel<false>, keyword_grid, dim3 (256), 0, st, C));
  HIP_TRY (launch (index_concat_check_kernel<true>, keyword_grid, dim3 (256), 0, st, C));
  HIP_TRY (launch (index_concat_finish_kernel, keyword_grid, dim3 (256), 0, st, C));
  /* the fill pass, by the room */
  if (d_out_text)
    HIP_TRY (launch (index_concat_fill_kernel, capped_grid (plan, (out_capacity + 255) / 256), dim3 (256), 0, st, C));
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_index_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity, uint64_t n_symbols, uint64_t n_texts,
                         uint64_t n_keywords, uint64_t post_capacity) {
  if (n_keywords >= (1ull << 32) || post_capacity >= (1ull << 31) ||
      !acm_gpu_tally_batch_tmp_bytes (plan, window_symbols, capacity, pair_capacity, n_symbols, n_texts))
    return 0;
  Carve c;
  rules_call_carve (c, plan, index_bytes (n_texts, n_keywords, post_capacity), capacity, pair_capacity, n_symbols, n_texts);
  return c.total ();
}

extern "C" int
acm_gpu_index_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint64_t window_symbols,
                      uint64_t capacity, uint64_t pair_capacity, uint64_t n_keywords, uint64_t text_base, uint64_t *d_post_ptr, uint32_t *d_post_text,
                      uint64_t *d_post_count, uint64_t post_capacity, uint64_t *d_nnz, uint64_t *d_forms, uint64_t *d_total, uint64_t *d_need,
                      uint64_t *d_need_pairs, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!index_args_ok (plan, n_texts, n_keywords, text_base, d_post_ptr, d_post_text, d_post_count, post_capacity, d_nnz) || !d_tmp || capacity == 0 ||
      capacity >= (1ull << 31) || pair_capacity == 0 || pair_capacity >= (1ull << 31))
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  const RulesCallRoom L = rules_call_carve (carve, plan, index_bytes (n_texts, n_keywords, post_capacity), capacity, pair_capacity, n_symbols, n_texts);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (const int rc = tally_then_evaluate (plan, d_text, n_symbols, d_offsets, n_texts, window_symbols, capacity, pair_capacity, L, d_post_ptr, d_nnz, d_total,
                                          d_need, d_need_pairs, stream, [&] {
                                            return index_transpose (plan, L.row_ptr, L.col, L.val, n_texts, n_keywords, text_base, d_post_ptr, d_post_text,
                                                                    d_post_count, post_capacity, d_nnz, d_forms, d_tmp, st, L.tb, capacity, pair_capacity);
                                          }))
    return rc;
  return n_texts == 0 ? index_empty (n_keywords, d_post_ptr, d_nnz, d_forms, st) : ACM_GPU_OK;
}

extern "C" int
acm_gpu_index_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, uint64_t text_base, uint64_t *post_ptr, uint64_t n_keywords,
                    uint32_t *post_text, uint64_t *post_count, uint64_t post_capacity, uint64_t *nnz, uint64_t *total) {
  if (!plan || !post_ptr || !nnz || n_keywords < plan->covered_keywords || n_keywords >= (1ull << 32) || text_base > (1ull << 32) ||
      text_base + n_texts > (1ull << 32) || post_capacity >= (1ull << 31) || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  const uint64_t n_symbols = offsets[n_texts];
  const bool fills = post_text && post_count && post_capacity;
  DeviceTemps temps;
  void *d_text = nullptr;
  uint64_t *d_off = nullptr, *d_post_ptr = nullptr, *d_post_count = nullptr, *d_res = nullptr; /* d_res: nnz, total, need, need_pairs */
  uint32_t *d_post_text = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  HOST_TRY (temps.get (&d_post_ptr, (n_keywords + 1) * 8));
  HOST_TRY (temps.get (&d_res, 32));
  if (fills) {
    HOST_TRY (temps.get (&d_post_text, (size_t)post_capacity * 4));
    HOST_TRY (temps.get (&d_post_count, (size_t)post_capacity * 8));
  }
  const uint64_t d_capacity = fills ? post_capacity : 0;
  uint64_t res[4] = { 0, 0, 0, 0 };
  if (const int rc = with_tally_rooms (
        plan, temps, n_symbols, d_res, res,
        [&] (uint64_t window, uint64_t capacity, uint64_t pairs) {
          return acm_gpu_index_tmp_bytes (plan, window, capacity, pairs, n_symbols, n_texts, n_keywords, d_capacity);
        },
        [&] (uint64_t window, uint64_t capacity, uint64_t pairs, void *d_tmp, size_t tmp_bytes) {
          return acm_gpu_index_device (plan, d_text, n_symbols, d_off, n_texts, window, capacity, pairs, n_keywords, text_base, d_post_ptr, d_post_text,
                                       d_post_count, d_capacity, d_res, nullptr, d_res + 1, d_res + 2, d_res + 3, d_tmp, tmp_bytes, nullptr);
        }))
    return rc;
  HOST_TRY (hipMemcpy (post_ptr, d_post_ptr, (n_keywords + 1) * 8, hipMemcpyDeviceToHost));
  *nnz = res[0];
  if (total)
    *total = res[1];
  if (!post_text || !post_count) /* the call only counts */
    return ACM_GPU_OK;
  if (res[0] > post_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (res[0]) {
    HOST_TRY (hipMemcpy (post_text, d_post_text, res[0] * 4, hipMemcpyDeviceToHost));
    HOST_TRY (hipMemcpy (post_count, d_post_count, res[0] * 8, hipMemcpyDeviceToHost));
  }
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ the co-occurrence matrix of a batch (include/acm_cooccur.h, dev_cooccur.h)
 * The passes that expand a count matrix on the device into its keyword pairs and reduce equal pairs, and
 * the sum of two such matrices; acm_gpu_cooccur_device runs the former behind acm_gpu_tally_batch_device. */
namespace {
/* what cooccur_carve derives beside K's pointers */
struct CooccurRoom {
  size_t zero_bytes = 0; /* control words and the texts' pair counts: the head of the scratch, cleared in front of every call */
  long long *p = nullptr, *pbase = nullptr; /* K's, as the sum takes them */
  unsigned long long *key[2] = { nullptr, nullptr }, *w[2] = { nullptr, nullptr }; /* the sort room and its second half */
  uint32_t *rank = nullptr;
  CubRoom cub;  /* the exclusive sums: n_texts + 1 pair counts, room + 1 marks */
  void *scan_tmp = nullptr, *sort_tmp = nullptr; /* the weights' inclusive sum, the radix sort */
  size_t scan_bytes = 0, sort_bytes = 0;
};

size_t
cooccur_scan_bytes (uint64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::InclusiveSum (nullptr, bytes, static_cast<unsigned long long *> (nullptr), static_cast<unsigned long long *> (nullptr), (int)n,
                                          nullptr);
  return bytes;
}

/* scratch of the radix sort over n slots, keys alone or pairs, whichever needs more */
size_t
cooccur_sort_bytes (uint64_t n) {
  size_t keys_only = 0;
  hipcub::DoubleBuffer<unsigned long long> k (nullptr, nullptr);
  (void)hipcub::DeviceRadixSort::SortKeys (nullptr, keys_only, k, (int)n, 0, 64, nullptr);
  return std::max (keys_only, index_sort_bytes (n));
}

/* n_texts = 0: ADD, which has no rows to count */
CooccurRoom
cooccur_carve (Carve &c, uint64_t n_texts, uint64_t cross_capacity, CoK &K) {
  CooccurRoom R;
  K.room = cross_capacity ? cross_capacity : 1;
  K.G.ctl = c.take<RulesCtl> (1);
  K.cctl = c.take<CoCtl> (1);
  R.p = c.take<long long> (n_texts + 1);
  R.zero_bytes = c.used;
  R.pbase = c.take<long long> (n_texts + 1);
  for (int h = 0; h < 2; h++) {
    R.key[h] = c.take<unsigned long long> ((size_t)K.room);
    R.w[h] = c.take<unsigned long long> ((size_t)K.room);
  }
  K.mark = c.take<uint32_t> ((size_t)K.room + 1);
  R.rank = c.take<uint32_t> ((size_t)K.room + 1);
  R.cub = cub_room (c, K.room + 1, n_texts + 1);
  R.scan_bytes = cooccur_scan_bytes (K.room);
  R.scan_tmp = c.take (R.scan_bytes + 16);
  R.sort_bytes = cooccur_sort_bytes (K.room);
  R.sort_tmp = c.take (R.sort_bytes + 16);
  K.p = reinterpret_cast<unsigned long long *> (R.p);
  K.pbase = reinterpret_cast<const unsigned long long *> (R.pbase);
  K.key = R.key[0];
  K.w = R.w[0];
  K.rank = R.rank;
  return R;
}

/* acm_gpu_cooccur_matrix_tmp_bytes behind its checks */
size_t
cooccur_bytes (uint64_t n_texts, uint64_t cross_capacity) {
  Carve c;
  CoK K{};
  cooccur_carve (c, n_texts, cross_capacity, K);
  return c.total ();
}

/* the matrix calls' own arguments */
bool
cooccur_args_ok (const ACMPlan *plan, uint64_t n_texts, uint64_t n_keywords, uint32_t flags, uint64_t cross_capacity, const uint64_t *d_co_ptr,
                 const uint32_t *d_co_col, const uint64_t *d_co_val, uint64_t out_capacity, const uint64_t *d_nnz, const uint64_t *d_cross,
                 const uint64_t *d_skipped) {
  return plan && n_texts < (1ull << 31) && n_keywords >= plan->covered_keywords && n_keywords < (1ull << 32) &&
         !(flags & ~(ACM_COOCCUR_PRODUCT | ACM_COOCCUR_DIAGONAL)) && cross_capacity < (1ull << 31) && out_capacity < (1ull << 31) && d_co_ptr && d_nnz &&
         d_cross && d_skipped && ((d_co_col && d_co_val) || (out_capacity == 0 && !d_co_col && !d_co_val));
}

/* without a text: every row is empty */
int
cooccur_empty (uint64_t n_keywords, uint64_t *d_co_ptr, uint64_t *d_nnz, uint64_t *d_cross, uint64_t *d_skipped, hipStream_t st) {
  HIP_TRY (hipMemsetAsync (d_co_ptr, 0, (n_keywords + 1) * 8, st));
  HIP_TRY (hipMemsetAsync (d_nnz, 0, 8, st));
  HIP_TRY (hipMemsetAsync (d_cross, 0, 8, st));
  HIP_TRY (hipMemsetAsync (d_skipped, 0, 8, st));
  return ACM_GPU_OK;
}

/* bits of a key's b-field: the fewest with 2^kb - 1 >= n_keywords, so that an all-ones field is no keyword */
uint32_t
cooccur_key_bits (uint64_t n_keywords) {
  uint32_t kb = 1;
  while (((1ull << kb) - 1) < n_keywords)
    kb++;
  return kb;
}

/* passes 4 to 7 of dev_cooccur.h over the room as pass 3 (or ADD's feed) filled it; weights: sort pairs and sum them */
int
cooccur_reduce (ACMPlan *plan, CoK &K, const CooccurRoom &L, bool weights, hipStream_t st) {
  const dim3 room_grid = capped_grid (plan, (K.room + 1 + 255) / 256);
  /* 4. */
  hipcub::DoubleBuffer<unsigned long long> keys (L.key[0], L.key[1]), vals (L.w[0], L.w[1]);
  size_t sort_bytes = L.sort_bytes;
  if (weights)
    HIP_TRY (hipcub::DeviceRadixSort::SortPairs (L.sort_tmp, sort_bytes, keys, vals, (int)K.room, 0, (int)(2 * K.kb), st));
  else
    HIP_TRY (hipcub::DeviceRadixSort::SortKeys (L.sort_tmp, sort_bytes, keys, (int)K.room, 0, (int)(2 * K.kb), st));
  K.skey = keys.Current ();
  K.start = reinterpret_cast<uint32_t *> (keys.Alternate ());
  HIP_TRY (launch (cooccur_heads_kernel, room_grid, dim3 (256), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.mark, L.rank, K.room + 1, st));
  /* 5. */
  if (weights) {
    size_t scan_bytes = L.scan_bytes;
    HIP_TRY (hipcub::DeviceScan::InclusiveSum (L.scan_tmp, scan_bytes, vals.Current (), vals.Alternate (), (int)K.room, st));
    K.wsum = vals.Alternate ();
  }
  /* 6. */
  HIP_TRY (launch (cooccur_ptr_kernel, capped_grid (plan, (K.n_keywords + 1 + 255) / 256), dim3 (256), 0, st, K));
  /* 7. (by the room: the host knows no more of nnz than that it is at most min (room, out_capacity)) */
  if (K.d_co_col) {
    HIP_TRY (launch (cooccur_starts_kernel, room_grid, dim3 (256), 0, st, K));
    HIP_TRY (launch (cooccur_fill_kernel, capped_grid (plan, (std::min (K.room, K.out_capacity) + 255) / 256), dim3 (256), 0, st, K));
  }
  return ACM_GPU_OK;
}

/* the passes of dev_cooccur.h on a matrix on the device; `tb` as rules_evaluate has it */
int
cooccur_build (ACMPlan *plan, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts, uint64_t n_keywords, uint32_t flags,
               uint64_t row_limit, uint64_t cross_capacity, uint64_t *d_co_ptr, uint32_t *d_co_col, uint64_t *d_co_val, uint64_t out_capacity,
               uint64_t *d_nnz, uint64_t *d_cross, uint64_t *d_skipped, void *d_tmp, hipStream_t st, const TbCtl *tb, uint64_t tb_capacity,
               uint64_t tb_pair_capacity) {
  Carve carve (d_tmp);
  CoK K{};
  const CooccurRoom L = cooccur_carve (carve, n_texts, cross_capacity, K);
  K.G.row_ptr = reinterpret_cast<const unsigned long long *> (d_row_ptr);
  K.G.n_texts = n_texts;
  K.G.tb = tb;
  K.G.tb_capacity = tb_capacity;
  K.G.tb_pair_capacity = tb_pair_capacity;
  K.G.error = error_word (plan);
  K.col = d_col;
  K.val = reinterpret_cast<const unsigned long long *> (d_val);
  K.n_keywords = n_keywords;
  K.row_limit = row_limit;
  K.cross_capacity = cross_capacity;
  K.out_capacity = out_capacity;
  K.flags = flags;
  K.kb = cooccur_key_bits (n_keywords);
  K.d_co_ptr = reinterpret_cast<unsigned long long *> (d_co_ptr);
  K.d_co_col = d_co_col;
  K.d_co_val = reinterpret_cast<unsigned long long *> (d_co_val);
  K.d_nnz = reinterpret_cast<unsigned long long *> (d_nnz);
  K.d_cross = reinterpret_cast<unsigned long long *> (d_cross);
  K.d_skipped = reinterpret_cast<unsigned long long *> (d_skipped);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  const dim3 text_grid = capped_grid (plan, (n_texts + 1 + 255) / 256);
  /* 1. */
  HIP_TRY (launch (rules_check_kernel, text_grid, dim3 (256), 0, st, K.G));
  /* 2. */
  HIP_TRY (launch (cooccur_count_kernel, text_grid, dim3 (256), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, L.p, L.pbase, n_texts + 1, st));
  HIP_TRY (launch (cooccur_finish_kernel, dim3 (1), dim3 (WAVE), 0, st, K));
  /* 3. */
  HIP_TRY (launch (cooccur_expand_kernel, capped_grid (plan, (K.room + 255) / 256), dim3 (256), 0, st, K));
  return cooccur_reduce (plan, K, L, (flags & ACM_COOCCUR_PRODUCT) != 0, st);
}
} // namespace

extern "C" size_t
acm_gpu_cooccur_matrix_tmp_bytes (const ACMPlan *plan, uint64_t n_texts, uint64_t n_keywords, uint64_t cross_capacity) {
  if (!plan || n_texts >= (1ull << 31) || n_keywords < plan->covered_keywords || n_keywords >= (1ull << 32) || cross_capacity >= (1ull << 31))
    return 0;
  return cooccur_bytes (n_texts, cross_capacity);
}

extern "C" int
acm_gpu_cooccur_matrix_device (ACMPlan *plan, const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_val, uint64_t n_texts, uint64_t n_keywords,
                               uint32_t flags, uint64_t row_limit, uint64_t cross_capacity, uint64_t *d_co_ptr, uint32_t *d_co_col, uint64_t *d_co_val,
                               uint64_t out_capacity, uint64_t *d_nnz, uint64_t *d_cross, uint64_t *d_skipped, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!cooccur_args_ok (plan, n_texts, n_keywords, flags, cross_capacity, d_co_ptr, d_co_col, d_co_val, out_capacity, d_nnz, d_cross, d_skipped))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0)
    return cooccur_empty (n_keywords, d_co_ptr, d_nnz, d_cross, d_skipped, st);
  if (!d_row_ptr || !d_tmp || tmp_bytes < cooccur_bytes (n_texts, cross_capacity))
    return ACM_GPU_E_ARG;
  return cooccur_build (plan, d_row_ptr, d_col, d_val, n_texts, n_keywords, flags, row_limit, cross_capacity, d_co_ptr, d_co_col, d_co_val, out_capacity,
                        d_nnz, d_cross, d_skipped, d_tmp, st, nullptr, 0, 0);
}

extern "C" size_t
acm_gpu_cooccur_add_tmp_bytes (const ACMPlan *plan, uint64_t n_keywords_b, uint64_t cross_capacity) {
  if (!plan || n_keywords_b >= (1ull << 32) || cross_capacity >= (1ull << 31))
    return 0;
  return cooccur_bytes (0, cross_capacity);
}

extern "C" int
acm_gpu_cooccur_add_device (ACMPlan *plan, const uint64_t *d_a_ptr, const uint32_t *d_a_col, const uint64_t *d_a_val, uint64_t n_keywords_a,
                            const uint64_t *d_b_ptr, const uint32_t *d_b_col, const uint64_t *d_b_val, uint64_t n_keywords_b, uint64_t cross_capacity,
                            uint64_t *d_out_ptr, uint32_t *d_out_col, uint64_t *d_out_val, uint64_t out_capacity, uint64_t *d_out_nnz, uint64_t *d_cross,
                            void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_a_ptr || !d_b_ptr || n_keywords_a > n_keywords_b || n_keywords_b >= (1ull << 32) || cross_capacity >= (1ull << 31) ||
      out_capacity >= (1ull << 31) || !d_out_ptr || !d_out_nnz || !d_cross ||
      !((d_out_col && d_out_val) || (out_capacity == 0 && !d_out_col && !d_out_val)) || !d_tmp || tmp_bytes < cooccur_bytes (0, cross_capacity))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  Carve carve (d_tmp);
  CoK K{};
  const CooccurRoom L = cooccur_carve (carve, 0, cross_capacity, K);
  K.G.error = error_word (plan);
  K.a_ptr = reinterpret_cast<const unsigned long long *> (d_a_ptr);
  K.b_ptr = reinterpret_cast<const unsigned long long *> (d_b_ptr);
  K.a_val = reinterpret_cast<const unsigned long long *> (d_a_val);
  K.b_val = reinterpret_cast<const unsigned long long *> (d_b_val);
  K.a_col = d_a_col;
  K.b_col = d_b_col;
  K.n_a = n_keywords_a;
  K.n_keywords = n_keywords_b;
  K.cross_capacity = cross_capacity;
  K.out_capacity = out_capacity;
  K.flags = ACM_COOCCUR_PRODUCT; /* (the later passes sum weights) */
  K.kb = cooccur_key_bits (n_keywords_b);
  K.d_co_ptr = reinterpret_cast<unsigned long long *> (d_out_ptr);
  K.d_co_col = d_out_col;
  K.d_co_val = reinterpret_cast<unsigned long long *> (d_out_val);
  K.d_nnz = reinterpret_cast<unsigned long long *> (d_out_nnz);
  K.d_cross = reinterpret_cast<unsigned long long *> (d_cross);
  HIP_TRY (hipMemsetAsync (d_tmp, 0, L.zero_bytes, st));
  /* the check of the pointer arrays (an address is formed from them only behind it), the room needed, the feed */
  HIP_TRY (launch (cooccur_add_check_kernel, capped_grid (plan, (n_keywords_b + 1 + 255) / 256), dim3 (256), 0, st, K));
  HIP_TRY (launch (cooccur_add_finish_kernel, dim3 (1), dim3 (WAVE), 0, st, K));
  HIP_TRY (launch (cooccur_add_feed_kernel, capped_grid (plan, (K.room + 255) / 256), dim3 (256), 0, st, K));
  return cooccur_reduce (plan, K, L, true, st);
}

extern "C" size_t
acm_gpu_cooccur_tmp_bytes (const ACMPlan *plan, uint64_t window_symbols, uint64_t capacity, uint64_t pair_capacity, uint64_t n_symbols, uint64_t n_texts,
                           uint64_t n_keywords, uint64_t cross_capacity) {
  if (n_keywords >= (1ull << 32) || cross_capacity >= (1ull << 31) ||
      !acm_gpu_tally_batch_tmp_bytes (plan, window_symbols, capacity, pair_capacity, n_symbols, n_texts) || n_keywords < plan->covered_keywords)
    return 0;
  Carve c;
  rules_call_carve (c, plan, cooccur_bytes (n_texts, cross_capacity), capacity, pair_capacity, n_symbols, n_texts);
  return c.total ();
}

extern "C" int
acm_gpu_cooccur_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint64_t window_symbols,
                        uint64_t capacity, uint64_t pair_capacity, uint64_t n_keywords, uint32_t flags, uint64_t row_limit, uint64_t cross_capacity,
                        uint64_t *d_co_ptr, uint32_t *d_co_col, uint64_t *d_co_val, uint64_t out_capacity, uint64_t *d_nnz, uint64_t *d_cross,
                        uint64_t *d_skipped, uint64_t *d_total, uint64_t *d_need, uint64_t *d_need_pairs, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!cooccur_args_ok (plan, n_texts, n_keywords, flags, cross_capacity, d_co_ptr, d_co_col, d_co_val, out_capacity, d_nnz, d_cross, d_skipped) || !d_tmp ||
      capacity == 0 || capacity >= (1ull << 31) || pair_capacity == 0 || pair_capacity >= (1ull << 31))
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  const RulesCallRoom L = rules_call_carve (carve, plan, cooccur_bytes (n_texts, cross_capacity), capacity, pair_capacity, n_symbols, n_texts);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (const int rc = tally_then_evaluate (plan, d_text, n_symbols, d_offsets, n_texts, window_symbols, capacity, pair_capacity, L, d_co_ptr, d_nnz, d_total,
                                          d_need, d_need_pairs, stream, [&] {
                                            return cooccur_build (plan, L.row_ptr, L.col, L.val, n_texts, n_keywords, flags, row_limit, cross_capacity,
                                                                  d_co_ptr, d_co_col, d_co_val, out_capacity, d_nnz, d_cross, d_skipped, d_tmp, st, L.tb,
                                                                  capacity, pair_capacity);
                                          }))
    return rc;
  return n_texts == 0 ? cooccur_empty (n_keywords, d_co_ptr, d_nnz, d_cross, d_skipped, st) : ACM_GPU_OK;
}

extern "C" int
acm_gpu_cooccur_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, uint64_t n_keywords, uint32_t flags, uint64_t row_limit,
                      uint64_t *co_ptr, uint32_t *co_col, uint64_t *co_val, uint64_t out_capacity, uint64_t *nnz, uint64_t *cross, uint64_t *skipped,
                      uint64_t *total) {
  if (!plan || !co_ptr || !nnz || n_keywords < plan->covered_keywords || n_keywords >= (1ull << 32) ||
      (flags & ~(ACM_COOCCUR_PRODUCT | ACM_COOCCUR_DIAGONAL)) || out_capacity >= (1ull << 31) || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  const uint64_t n_symbols = offsets[n_texts];
  const bool fills = co_col && co_val && out_capacity;
  DeviceTemps temps;
  void *d_text = nullptr;
  uint64_t *d_off = nullptr, *d_co_ptr = nullptr, *d_co_val = nullptr, *d_res = nullptr; /* d_res: nnz, total, need, need_pairs, cross, skipped */
  uint32_t *d_co_col = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  HOST_TRY (temps.get (&d_co_ptr, (n_keywords + 1) * 8));
  HOST_TRY (temps.get (&d_res, 48));
  HOST_TRY (hipMemset (d_res, 0, 48));
  if (fills) {
    HOST_TRY (temps.get (&d_co_col, (size_t)out_capacity * 4));
    HOST_TRY (temps.get (&d_co_val, (size_t)out_capacity * 8));
  }
  const uint64_t d_capacity = fills ? out_capacity : 0;
  /* the cross room: a guess, then what the device reported, which is exact */
  uint64_t cross_capacity = std::min<uint64_t> (std::max<uint64_t> (1ull << 16, 4 * n_texts), (1ull << 31) - 1);
  uint64_t res[4] = { 0, 0, 0, 0 }, more[2] = { 0, 0 };
  for (int attempt = 0;; attempt++) {
    if (const int rc = with_tally_rooms (
          plan, temps, n_symbols, d_res, res,
          [&] (uint64_t window, uint64_t capacity, uint64_t pairs) {
            return acm_gpu_cooccur_tmp_bytes (plan, window, capacity, pairs, n_symbols, n_texts, n_keywords, cross_capacity);
          },
          [&] (uint64_t window, uint64_t capacity, uint64_t pairs, void *d_tmp, size_t tmp_bytes) {
            return acm_gpu_cooccur_device (plan, d_text, n_symbols, d_off, n_texts, window, capacity, pairs, n_keywords, flags, row_limit, cross_capacity,
                                           d_co_ptr, d_co_col, d_co_val, d_capacity, d_res, d_res + 4, d_res + 5, d_res + 1, d_res + 2, d_res + 3, d_tmp,
                                           tmp_bytes, nullptr);
          }))
      return rc;
    HOST_TRY (hipMemcpy (more, d_res + 4, 16, hipMemcpyDeviceToHost));
    if (more[0] <= cross_capacity)
      break;
    if (more[0] >= (1ull << 31)) /* more pair instances than one call holds */
      return ACM_GPU_E_NOMEM;
    if (attempt) /* (the second room is what the first attempt asked for: never expected) */
      return ACM_GPU_E_INTERNAL;
    cross_capacity = more[0];
  }
  HOST_TRY (hipMemcpy (co_ptr, d_co_ptr, (n_keywords + 1) * 8, hipMemcpyDeviceToHost));
  *nnz = res[0];
  if (cross)
    *cross = more[0];
  if (skipped)
    *skipped = more[1];
  if (total)
    *total = res[1];
  if (!co_col || !co_val) /* the call only counts */
    return ACM_GPU_OK;
  if (res[0] > out_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (res[0]) {
    HOST_TRY (hipMemcpy (co_col, d_co_col, res[0] * 4, hipMemcpyDeviceToHost));
    HOST_TRY (hipMemcpy (co_val, d_co_val, res[0] * 8, hipMemcpyDeviceToHost));
  }
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ leftmost-longest selection (include/acm_gpu.h, dev_select.h)
 * The passes over a record set in canonical order; acm_gpu_scan_select_device runs them behind the
 * ordered scan. */
namespace {
/* what select_carve derives beside K's pointers */
struct SelectRoom {
  uint32_t *chunk_begin = nullptr; /* K.chunk_begin, for the sum that writes it */
  CubRoom cub;
  size_t work_bytes = 0; /* of K.cand: the order pass's scratch; the candidates take its place when the order is made */
};
/* nothing here depends on the environment: the maps and the tiles' words are sized for every T */
SelectRoom
select_carve (Carve &c, const ACMPlan *plan, uint64_t capacity, uint64_t span, SelectK &K) {
  SelectRoom R;
  K.n_chunks = (capacity + SELECT_CHUNK - 1) / SELECT_CHUNK;
  R.work_bytes = std::max (acm_gpu_order_tmp_bytes (plan, capacity, span), (size_t)capacity * sizeof (ACMRecord) + 256);
  K.ctl = c.take<SelectCtl> (1);
  K.chunk_count = c.take<uint32_t> (K.n_chunks + 1);
  K.chunk_begin = R.chunk_begin = c.take<uint32_t> (K.n_chunks + 1);
  R.cub = cub_room (c, K.n_chunks + 1, 0);
  K.map = c.take<uint32_t> ((size_t)capacity + SELECT_TILE_MAX); /* tiles x E <= capacity + T words */
  K.tile_entry = c.take<uint32_t> ((size_t)capacity / SELECT_TILE_MIN + 1);
  K.tile_base = c.take<uint32_t> ((size_t)capacity / SELECT_TILE_MIN + 1);
  K.keyed = c.take<ACMRecord> ((size_t)(capacity ? capacity : 1));
  K.cand = reinterpret_cast<ACMRecord *> (c.take (R.work_bytes));
  return R;
}

/* ACM_GPU_SELECT_TILE=<candidates>: T (tests) */
uint32_t
select_tile (void) {
  return tunable ("ACM_GPU_SELECT_TILE", SELECT_TILE_DEFAULT, SELECT_TILE_MIN, SELECT_TILE_MAX, Tune::Any);
}

/* ACM_GPU_SELECT=walk: every plan takes the general form (experiments, tests) */
bool
select_tiled_form (const ACMPlan *plan, uint32_t tile) {
  const bool walk = getenv ("ACM_GPU_SELECT") && strcmp (getenv ("ACM_GPU_SELECT"), "walk") == 0;
  return !walk && plan_lmax (plan) <= tile;
}

/* no record to pass on (select, words): a count that came in stays -- it says what room the records
 * need --, else the count is 0 */
int
no_record (ACMPlan *plan, const uint64_t *d_n, uint64_t *d_count, hipStream_t st) {
  HIP_TRY (hipSetDevice (plan->device));
  if (!d_n)
    HIP_TRY (hipMemsetAsync (d_count, 0, 8, st));
  else if (d_n != d_count)
    HIP_TRY (hipMemcpyAsync (d_count, d_n, 8, hipMemcpyDeviceToDevice, st));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_select_form (const ACMPlan *plan) {
  if (!plan)
    return ACM_GPU_E_ARG;
  return select_tiled_form (plan, select_tile ()) ? ACM_GPU_SELECT_FORM_TILED : ACM_GPU_SELECT_FORM_WALK;
}

extern "C" size_t
acm_gpu_select_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t span) {
  if (!plan || capacity >= (1ull << 31))
    return 0;
  Carve c;
  SelectK K{};
  select_carve (c, plan, capacity, span, K);
  return c.total ();
}

extern "C" int
acm_gpu_select_records_device (ACMPlan *plan, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, uint64_t pos_lo, uint64_t span,
                               ACMRecord *d_out, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || n >= (1ull << 31) || (n && (!d_records || !d_out || !d_tmp || span == 0)))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n == 0) /* (no room) */
    return no_record (plan, d_n, d_count, st);
  Carve carve (d_tmp);
  SelectK K{};
  const SelectRoom L = select_carve (carve, plan, n, span, K);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.in = d_records;
  K.capacity = n;
  K.n_dev = reinterpret_cast<const unsigned long long *> (d_n);
  K.pos_lo = pos_lo;
  K.span = span;
  K.lmax = plan_lmax (plan);
  K.T = select_tile ();
  K.E = K.lmax < K.T ? K.lmax : K.T;
  K.max_tiles = (n + K.T - 1) / K.T;
  K.out = d_out;
  K.d_count = reinterpret_cast<unsigned long long *> (d_count);
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (SelectCtl), st));
  /* a. keys, the records that break the contract out, the order by (start, length descending) */
  HIP_TRY (launch (select_key_kernel, capped_grid (plan, (n + SELECT_THREADS - 1) / SELECT_THREADS), dim3 (SELECT_THREADS), 0, st, K));
  HIP_TRY (launch (select_drop_kernel, dim3 (1), dim3 (SELECT_THREADS), 0, st, K));
  if (order_by_buckets (plan, order_layout (plan, n, span))) {
    const int rc = order_records (plan, K.keyed, n, &K.ctl->n, pos_lo, span, K.cand, L.work_bytes, stream);
    if (rc)
      return rc;
  } else {
    /* record sets the bucket passes do not take (positions past 2^40; ACM_GPU_ORDER=radix): the count
     * comes to the host for the radix sort, as in acm_gpu_scan_ordered_device */
    uint64_t kept = 0;
    HIP_TRY (hipMemcpyAsync (&kept, &K.ctl->n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY (hipStreamSynchronize (st));
    if (kept > 1) {
      const int rc = order_records (plan, K.keyed, kept, nullptr, pos_lo, span, K.cand, L.work_bytes, stream);
      if (rc)
        return rc;
    }
  }
  /* b. the candidates */
  HIP_TRY (launch (select_cand_kernel<false>, capped_grid (plan, K.n_chunks + 1), dim3 (SELECT_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.chunk_count, L.chunk_begin, K.n_chunks + 1, st));
  HIP_TRY (launch (select_cand_kernel<true>, capped_grid (plan, K.n_chunks + 1), dim3 (SELECT_THREADS), 0, st, K));
  if (!select_tiled_form (plan, K.T)) { /* f. */
    HIP_TRY (launch (select_walk_kernel, dim3 (1), dim3 (WAVE), 0, st, K));
    return ACM_GPU_OK;
  }
  /* c. d. e. */
  const size_t lds = select_tile_lds (K.T);
  HIP_TRY (launch (select_tile_kernel<false>, capped_grid (plan, K.max_tiles), dim3 (SELECT_THREADS), lds, st, K));
  HIP_TRY (launch (select_resolve_kernel, dim3 (1), dim3 (SELECT_THREADS), 0, st, K));
  HIP_TRY (launch (select_tile_kernel<true>, capped_grid (plan, K.max_tiles), dim3 (SELECT_THREADS), lds, st, K));
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_scan_select_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols) {
  if (!plan || capacity >= (1ull << 31))
    return 0;
  /* (the scan's scratch is free again when the selection begins: it reads d_records) */
  return std::max (acm_gpu_scan_ordered_tmp_bytes (plan, capacity, n_symbols), acm_gpu_select_tmp_bytes (plan, capacity, n_symbols));
}

extern "C" int
acm_gpu_scan_select_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, ACMRecord *d_records, uint64_t capacity,
                            uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || capacity >= (1ull << 31) || (n_symbols && !d_text) || (capacity && (!d_records || !d_tmp)))
    return ACM_GPU_E_ARG;
  if (capacity && tmp_bytes < acm_gpu_scan_select_tmp_bytes (plan, capacity, n_symbols))
    return ACM_GPU_E_ARG;
  int rc = acm_gpu_scan_ordered_device (plan, d_text, n_symbols, 0, pos_base, d_records, capacity, d_count, d_tmp, tmp_bytes, stream);
  if (rc || capacity == 0 || n_symbols == 0) /* (no room: *d_count says what the records need; no text: 0) */
    return rc;
  return acm_gpu_select_records_device (plan, d_records, capacity, d_count, pos_base, n_symbols, d_records, d_count, d_tmp, tmp_bytes, stream);
}

extern "C" int
acm_gpu_scan_select_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, ACMRecord *records, uint64_t capacity,
                          uint64_t *n_found) {
  if (!plan || !n_found || capacity >= (1ull << 31) || (n_symbols && !text) || (capacity && !records))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const size_t tmp_bytes = acm_gpu_scan_select_tmp_bytes (plan, capacity, n_symbols);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_count = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_count, 8));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  const int rc = acm_gpu_scan_select_device (plan, d_text, n_symbols, pos_base, d_rec, capacity, d_count, d_tmp, tmp_bytes, nullptr);
  return download_records (rc, d_count, d_rec, records, capacity, n_found);
}

/* ------------------------------------------------------------------ minimum-cost tiling (include/acm_segment.h, dev_segment.h)
 * The passes over a record set in canonical order; acm_gpu_scan_segment_device runs them behind the
 * ordered scan or the batch scan. */
namespace {
/* what segment_carve derives beside K's pointers */
struct SegmentRoom {
  uint32_t *tile_begin = nullptr; /* K.tile_begin, for the sums that write it */
  CubRoom cub;
};
/* ACM_GPU_SEGMENT_TILE=<records>: the tile of the group and compaction passes, a multiple of 64 (tests) */
uint32_t
segment_tile (void) {
  return tunable ("ACM_GPU_SEGMENT_TILE", SEGMENT_TILE_DEFAULT, SEGMENT_TILE_MIN, SEGMENT_TILE_MAX, Tune::MultWave);
}

/* ACM_GPU_SEGMENT_LONG=<records>: the groups of so many records take the wave form (tests) */
uint32_t
segment_long (void) {
  return tunable ("ACM_GPU_SEGMENT_LONG", SEGMENT_LONG_DEFAULT, SEGMENT_LONG_MIN, SEGMENT_LONG_MAX, Tune::Any);
}

SegmentRoom
segment_carve (Carve &c, uint64_t capacity, SegmentK &K) {
  SegmentRoom R;
  const size_t room = (size_t)(capacity ? capacity : 1);
  K.tile = segment_tile ();
  K.n_tiles = (capacity + K.tile - 1) / K.tile;
  K.S.ctl = c.take<SelectCtl> (1);
  K.ctl = c.take<SegmentCtl> (1);
  K.tile_min = c.take<unsigned long long> (K.n_tiles + 1);
  K.tile_count = c.take<uint32_t> (K.n_tiles + 1);
  K.tile_begin = R.tile_begin = c.take<uint32_t> (K.n_tiles + 1);
  R.cub = cub_room (c, K.n_tiles + 1, 0);
  K.S.keyed = c.take<ACMRecord> (room);
  K.V = c.take<unsigned long long> (room);
  K.mark = c.take<uint32_t> (room);
  K.group_first = c.take<uint32_t> (room);
  K.prev = c.take<uint32_t> (room);
  K.choice = c.take<uint32_t> (room);
  K.cfirst = c.take<uint32_t> (room);
  K.long_list = c.take<uint32_t> (room);
  return R;
}

/* what every entry checks of the cost table's shape (the values are the device's to check, or the host entry's) */
bool
segment_args_ok (const uint32_t *cost, uint64_t n_keywords, uint32_t gap_cost) {
  return gap_cost < SEGMENT_COST_LIMIT && n_keywords < (1ull << 32) && (cost || n_keywords == 0);
}
} // namespace

extern "C" size_t
acm_gpu_segment_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t span) {
  (void)span; /* (no order pass: the scratch goes by the records alone) */
  if (!plan || capacity >= (1ull << 31))
    return 0;
  Carve c;
  SegmentK K{};
  segment_carve (c, capacity, K);
  return c.total ();
}

extern "C" int
acm_gpu_segment_records_device (ACMPlan *plan, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, uint64_t pos_lo, uint64_t span,
                                const uint32_t *d_cost, uint64_t n_keywords, uint32_t gap_cost, ACMRecord *d_out, uint64_t *d_count,
                                uint64_t *d_sums, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || n >= (1ull << 31) || (n && (!d_records || !d_out || !d_tmp || span == 0)) || !segment_args_ok (d_cost, n_keywords, gap_cost))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n == 0) { /* (no room) */
    if (const int rc = no_record (plan, d_n, d_count, st))
      return rc;
    if (d_sums)
      HIP_TRY (hipMemsetAsync (d_sums, 0, 16, st));
    return ACM_GPU_OK;
  }
  Carve carve (d_tmp);
  SegmentK K{};
  const SegmentRoom L = segment_carve (carve, n, K);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.S.in = d_records;
  K.S.capacity = n;
  K.S.n_dev = reinterpret_cast<const unsigned long long *> (d_n);
  K.S.pos_lo = pos_lo;
  K.S.span = span;
  K.S.lmax = plan_lmax (plan);
  K.S.error = error_word (plan);
  K.cost = d_cost;
  K.n_keywords = n_keywords;
  K.gap = gap_cost;
  K.long_min = segment_long ();
  K.out = d_out;
  K.d_count = reinterpret_cast<unsigned long long *> (d_count);
  K.d_sums = reinterpret_cast<unsigned long long *> (d_sums);
  HIP_TRY (hipMemsetAsync (K.S.ctl, 0, sizeof (SelectCtl), st));
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (SegmentCtl), st));
  const dim3 threads (SEGMENT_THREADS), per_record = capped_grid (plan, (n + SEGMENT_THREADS - 1) / SEGMENT_THREADS),
                                        per_tile = capped_grid (plan, K.n_tiles + 1);
  /* a. SELECT's keys and contract, then the keyword ids and the costs */
  HIP_TRY (launch (select_key_kernel, per_record, threads, 0, st, K.S));
  HIP_TRY (launch (select_drop_kernel, dim3 (1), threads, 0, st, K.S));
  HIP_TRY (launch (segment_check_kernel, capped_grid (plan, (std::max (n, n_keywords) + SEGMENT_THREADS - 1) / SEGMENT_THREADS), threads, 0, st, K));
  /* b. the groups */
  HIP_TRY (launch (segment_min_kernel, per_tile, threads, 0, st, K));
  HIP_TRY (launch (segment_carry_kernel, dim3 (1), threads, 0, st, K));
  HIP_TRY (launch (segment_flag_kernel, per_tile, threads, 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.tile_count, L.tile_begin, K.n_tiles + 1, st));
  HIP_TRY (launch (segment_place_kernel<false>, per_tile, threads, 0, st, K));
  /* c. d. e. */
  HIP_TRY (launch (segment_link_kernel, per_record, threads, 0, st, K));
  HIP_TRY (launch (segment_lane_kernel, per_record, threads, 0, st, K));
  HIP_TRY (launch (segment_wave_kernel, capped_grid (plan, (n + K.long_min - 1) / K.long_min), dim3 (WAVE), 0, st, K));
  /* f. */
  HIP_TRY (launch (segment_count_kernel, per_tile, threads, 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.tile_count, L.tile_begin, K.n_tiles + 1, st));
  HIP_TRY (launch (segment_place_kernel<true>, per_tile, threads, 0, st, K));
  HIP_TRY (launch (segment_finish_kernel, dim3 (1), dim3 (WAVE), 0, st, K));
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_scan_segment_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || capacity >= (1ull << 31))
    return 0;
  /* (one room for both forms of the call: the scan's scratch is free again when the passes begin, they read d_records) */
  const size_t scans = std::max (acm_gpu_scan_ordered_tmp_bytes (plan, capacity, n_symbols), acm_gpu_scan_batch_tmp_bytes (plan, capacity, n_symbols, n_texts));
  return std::max (scans, acm_gpu_segment_tmp_bytes (plan, capacity, n_symbols));
}

extern "C" int
acm_gpu_scan_segment_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                             const uint32_t *d_cost, uint64_t n_keywords, uint32_t gap_cost, ACMRecord *d_records, uint64_t capacity,
                             uint64_t *d_count, uint64_t *d_sums, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || capacity >= (1ull << 31) || (n_symbols && !d_text) || (capacity && (!d_records || !d_tmp)) ||
      (d_offsets && (pos_base || n_texts >= (1ull << 31))) || !segment_args_ok (d_cost, n_keywords, gap_cost) || n_keywords < plan->covered_keywords)
    return ACM_GPU_E_ARG;
  if (capacity && tmp_bytes < acm_gpu_scan_segment_tmp_bytes (plan, capacity, n_symbols, n_texts))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  if (d_sums) /* (what stays when the passes do not run: no room, no text) */
    HIP_TRY (hipMemsetAsync (d_sums, 0, 16, static_cast<hipStream_t> (stream)));
  int rc;
  if (!d_offsets)
    rc = acm_gpu_scan_ordered_device (plan, d_text, n_symbols, 0, pos_base, d_records, capacity, d_count, d_tmp, tmp_bytes, stream);
  else
    rc = acm_gpu_scan_batch_device (plan, d_text, n_symbols, d_offsets, n_texts, d_records, nullptr, nullptr, capacity, d_count, d_tmp, tmp_bytes, stream);
  if (rc || capacity == 0 || n_symbols == 0) /* (no room: *d_count says what the records need; no text: 0) */
    return rc;
  return acm_gpu_segment_records_device (plan, d_records, capacity, d_count, pos_base, n_symbols, d_cost, n_keywords, gap_cost, d_records, d_count,
                                         d_sums, d_tmp, tmp_bytes, stream);
}

extern "C" int
acm_gpu_scan_segment_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                           const uint32_t *cost, uint64_t n_keywords, uint32_t gap_cost, ACMRecord *records, uint64_t capacity, uint64_t *n_found,
                           uint64_t sums[2]) {
  if (!plan || !n_found || capacity >= (1ull << 31) || (n_symbols && !text) || (capacity && !records) || (offsets && pos_base) ||
      !segment_args_ok (cost, n_keywords, gap_cost) || n_keywords < plan->covered_keywords || !optional_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k < n_keywords; k++)
    if (cost[k] >= SEGMENT_COST_LIMIT)
      return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const size_t tmp_bytes = acm_gpu_scan_segment_tmp_bytes (plan, capacity, n_symbols, n_texts);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_res = nullptr, *d_off = nullptr; /* d_res: the count, the sums */
  uint32_t *d_cost = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_res, 24));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  HOST_TRY (temps.get (&d_cost, n_keywords * 4));
  if (n_keywords)
    HOST_TRY (hipMemcpy (d_cost, cost, n_keywords * 4, hipMemcpyHostToDevice));
  if (offsets)
    HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  const int rc = acm_gpu_scan_segment_device (plan, d_text, n_symbols, pos_base, d_off, n_texts, d_cost, n_keywords, gap_cost, d_rec, capacity, d_res,
                                              d_res + 1, d_tmp, tmp_bytes, nullptr);
  return download_records (rc, d_res, d_rec, records, capacity, n_found, nullptr, [&] (uint64_t) -> int {
    if (sums)
      HOST_TRY (hipMemcpy (sums, d_res + 1, 16, hipMemcpyDeviceToHost));
    return (int)ACM_GPU_OK;
  });
}

/* ------------------------------------------------------------------ search-and-replace (include/acm_gpu.h, dev_replace.h)
 * The passes behind a selection: validate and measure, the prefix over the chunks and the records'
 * places in the output, the output itself. */
namespace {
/* what replace_carve derives beside K's pointers */
struct ReplaceRoom {
  long long *chunk_begin = nullptr; /* K.chunk_begin, for the sum that writes it */
  CubRoom cub;
};
ReplaceRoom
replace_carve (Carve &c, uint64_t capacity, ReplaceK &K) {
  ReplaceRoom R;
  K.n_chunks = (capacity + REPLACE_CHUNK - 1) / REPLACE_CHUNK;
  K.ctl = c.take<ReplaceCtl> (1);
  K.chunk_sum = c.take<long long> (K.n_chunks + 1);
  K.chunk_begin = R.chunk_begin = c.take<long long> (K.n_chunks + 1);
  R.cub = cub_room (c, 0, K.n_chunks + 1);
  K.out_start = c.take<long long> ((size_t)(capacity ? capacity : 1));
  return R;
}

/* table mode: the table has an entry for every keyword the plan can report */
bool
replace_table_covers (const ACMPlan *plan, const uint64_t *repl_off, uint64_t n_keywords) {
  return !repl_off || n_keywords >= plan->covered_keywords;
}
} // namespace

extern "C" size_t
acm_gpu_replace_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_symbols) {
  (void)n_symbols; /* (the passes keep nothing per symbol) */
  if (!plan || n_or_capacity >= (1ull << 31))
    return 0;
  Carve c;
  ReplaceK K{};
  replace_carve (c, n_or_capacity, K);
  return c.total ();
}

namespace {
/* the passes over a selection of n records, or of *d_n in a room of n */
int
replace_records (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const ACMRecord *d_sel, uint64_t n,
                 const uint64_t *d_n, const void *d_repl_data, const uint64_t *d_repl_off, uint64_t n_keywords, void *d_out, uint64_t out_capacity,
                 uint64_t *d_out_symbols, int64_t *d_out_start, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_out_symbols || !d_tmp || n >= (1ull << 31) || (n_symbols && !d_text) || (out_capacity && !d_out) || (n && !d_sel) ||
      (!d_repl_off && !d_repl_data) || n_keywords >= (1ull << 32))
    return ACM_GPU_E_ARG;
  const uint32_t sb = plan->text_sym_bytes;
  if (!symbols_ok (d_text, n_symbols, sb) || !symbols_ok (d_out, out_capacity, sb) || reinterpret_cast<uintptr_t> (d_repl_data) % sb ||
      !apart (d_text, n_symbols, d_out, out_capacity, sb))
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  ReplaceK K{};
  const ReplaceRoom L = replace_carve (carve, n, K);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  K.sel = d_sel;
  K.capacity = n;
  K.n_dev = reinterpret_cast<const unsigned long long *> (d_n);
  K.text = static_cast<const unsigned char *> (d_text);
  K.n_symbols = n_symbols;
  K.pos_base = pos_base;
  K.sb = sb;
  /* ACM_GPU_REPLACE_TILE=<bytes of output>: pass c's tile, a multiple of 16 (tests) */
  K.tile_words = tunable ("ACM_GPU_REPLACE_TILE", REPLACE_TILE_DEFAULT, REPLACE_TILE_MIN, REPLACE_TILE_MAX, Tune::Mult16) / 16;
  K.repl = static_cast<const unsigned char *> (d_repl_data);
  K.repl_off = reinterpret_cast<const unsigned long long *> (d_repl_off);
  K.n_keywords = n_keywords;
  K.d_out_start = reinterpret_cast<long long *> (d_out_start);
  K.out = static_cast<unsigned char *> (d_out);
  K.out_capacity = out_capacity;
  K.d_out_symbols = reinterpret_cast<unsigned long long *> (d_out_symbols);
  K.error = error_word (plan);
  const bool mask = d_repl_off == nullptr;
  const dim3 block (REPLACE_THREADS);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (ReplaceCtl), st));
  /* a. */
  const dim3 chunks_grid = capped_grid (plan, std::max (K.n_chunks + 1, mask ? (uint64_t)0 : (n_keywords + REPLACE_THREADS - 1) / REPLACE_THREADS));
  HIP_TRY (mask ? launch (replace_measure_kernel<true>, chunks_grid, block, 0, st, K) : launch (replace_measure_kernel<false>, chunks_grid, block, 0, st, K));
  /* b. */
  HIP_TRY (exclusive_sum (L.cub, K.chunk_sum, L.chunk_begin, K.n_chunks + 1, st));
  const dim3 starts_grid = capped_grid (plan, K.n_chunks);
  HIP_TRY (mask ? launch (replace_starts_kernel<true>, starts_grid, block, 0, st, K) : launch (replace_starts_kernel<false>, starts_grid, block, 0, st, K));
  /* c. the grid by the room of the output, not by what the passes found */
  const dim3 tiles_grid = capped_grid (plan, (out_capacity * sb + 15 + 16) / ((uint64_t)K.tile_words * 16) + 1);
  HIP_TRY (mask ? launch (replace_build_kernel<true>, tiles_grid, block, 0, st, K) : launch (replace_build_kernel<false>, tiles_grid, block, 0, st, K));
  return ACM_GPU_OK;
}

} // namespace

extern "C" int
acm_gpu_replace_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const ACMRecord *d_sel,
                                uint64_t n, const uint64_t *d_n, const void *d_repl_data, const uint64_t *d_repl_off, uint64_t n_keywords,
                                void *d_out, uint64_t out_capacity, uint64_t *d_out_symbols, int64_t *d_out_start, void *d_tmp, size_t tmp_bytes,
                                void *stream) {
  if (!plan || n >= (1ull << 31))
    return ACM_GPU_E_ARG;
  return replace_records (plan, d_text, n_symbols, pos_base, d_sel, n, d_n, d_repl_data, d_repl_off, n_keywords, d_out,
                          out_capacity, d_out_symbols, d_out_start, d_tmp, tmp_bytes, stream);
}

extern "C" size_t
acm_gpu_scan_replace_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols) {
  if (!plan || capacity >= (1ull << 31))
    return 0;
  /* (the selection has ended when the replace passes begin: they read d_records) */
  return std::max (acm_gpu_scan_select_tmp_bytes (plan, capacity, n_symbols), acm_gpu_replace_tmp_bytes (plan, capacity, n_symbols));
}

extern "C" int
acm_gpu_scan_replace_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, ACMRecord *d_records, uint64_t capacity,
                             uint64_t *d_count, const void *d_repl_data, const uint64_t *d_repl_off, uint64_t n_keywords, void *d_out,
                             uint64_t out_capacity, uint64_t *d_out_symbols, int64_t *d_out_start, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || !d_out_symbols || !d_tmp || capacity >= (1ull << 31) || (n_symbols && !d_text) || (capacity && !d_records) ||
      (out_capacity && !d_out) || (!d_repl_off && !d_repl_data) || !replace_table_covers (plan, d_repl_off, n_keywords))
    return ACM_GPU_E_ARG;
  if (tmp_bytes < acm_gpu_scan_replace_tmp_bytes (plan, capacity, n_symbols))
    return ACM_GPU_E_ARG;
  const int rc = acm_gpu_scan_select_device (plan, d_text, n_symbols, pos_base, d_records, capacity, d_count, d_tmp, tmp_bytes, stream);
  if (rc)
    return rc;
  return replace_records (plan, d_text, n_symbols, pos_base, d_records, capacity, d_count, d_repl_data, d_repl_off, n_keywords, d_out, out_capacity,
                          d_out_symbols, d_out_start, d_tmp, tmp_bytes, stream);
}

extern "C" int
acm_gpu_scan_replace_host (ACMPlan *plan, const void *text, uint64_t n_symbols, const void *repl_data, const uint64_t *repl_off, uint64_t n_keywords,
                           void *out, uint64_t out_capacity, uint64_t *out_symbols, uint64_t *n_replaced) {
  if (!plan || !out_symbols || (n_symbols && !text) || (out_capacity && !out) || (!repl_off && !repl_data) ||
      !replace_table_covers (plan, repl_off, n_keywords) || n_keywords >= (1ull << 32))
    return ACM_GPU_E_ARG;
  const uint32_t sb = plan->text_sym_bytes;
  if (repl_off) {
    if (repl_off[0] != 0)
      return ACM_GPU_E_ARG;
    for (uint64_t k = 0; k < n_keywords; k++)
      if (repl_off[k] > repl_off[k + 1])
        return ACM_GPU_E_ARG;
    if (repl_off[n_keywords] && !repl_data)
      return ACM_GPU_E_ARG;
  }
  HIP_TRY (hipSetDevice (plan->device));
  const size_t obytes = (size_t)out_capacity * sb;
  const size_t rbytes = (size_t)(repl_off ? repl_off[n_keywords] : 1) * sb;
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr, *d_repl = nullptr, *d_out = nullptr;
  uint64_t *d_res = nullptr, *d_off = nullptr; /* d_res: the count, the output's symbols */
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_res, 16));
  uint64_t matches = 0;
  int rc = count_first (plan, d_text, n_symbols, d_res, &matches);
  if (rc)
    return rc;
  const size_t tmp_bytes = acm_gpu_scan_replace_tmp_bytes (plan, matches, n_symbols);
  HOST_TRY (temps.get (&d_rec, matches * 16));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  HOST_TRY (temps.get (&d_repl, rbytes));
  HOST_TRY (temps.get (&d_out, obytes));
  if (rbytes && repl_data)
    HOST_TRY (hipMemcpy (d_repl, repl_data, rbytes, hipMemcpyHostToDevice));
  if (repl_off) {
    HOST_TRY (temps.get (&d_off, (n_keywords + 1) * 8));
    HOST_TRY (hipMemcpy (d_off, repl_off, (n_keywords + 1) * 8, hipMemcpyHostToDevice));
  }
  rc = settle (plan, acm_gpu_scan_replace_device (plan, d_text, n_symbols, 0, d_rec, matches, d_res, d_repl, d_off, n_keywords, d_out, out_capacity,
                                                  d_res + 1, nullptr, d_tmp, tmp_bytes, nullptr), true);
  if (rc)
    return rc;
  uint64_t res[2] = { 0, 0 };
  HOST_TRY (hipMemcpy (res, d_res, 16, hipMemcpyDeviceToHost));
  if (res[0] > matches) /* (the scan found more than the count said: never expected) */
    return ACM_GPU_E_INTERNAL;
  *out_symbols = res[1];
  if (n_replaced)
    *n_replaced = res[0];
  if (res[1] > out_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (res[1])
    HOST_TRY (hipMemcpy (out, d_out, (size_t)res[1] * sb, hipMemcpyDeviceToHost));
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ tokenising (include/acm_gpu.h, dev_tokens.h)
 * The passes behind a selection: validate, count the token starts per tile of the text, the prefix
 * over the tiles, the tokens themselves. */
namespace {
/* what tokens_carve derives beside K's pointers */
struct TokensRoom {
  bool ok = false; /* false: a text of more tiles than the prefix sum can count (its entries are an int's), nothing carved */
  long long *tile_begin = nullptr; /* K.tile_begin, for the sum that writes it */
  CubRoom cub;
};
TokensRoom
tokens_carve (Carve &c, uint64_t n_symbols, TokensK &K) {
  TokensRoom R;
  /* ACM_GPU_TOKENS_TILE=<symbols>: the tile of the passes, a multiple of 64 (tests) */
  K.tile = tunable ("ACM_GPU_TOKENS_TILE", TOKENS_TILE_DEFAULT, TOKENS_TILE_MIN, TOKENS_TILE_MAX, Tune::MultWave);
  K.n_tiles = (n_symbols + K.tile - 1) / K.tile;
  if (K.n_tiles + 1 >= (1ull << 31))
    return R;
  R.ok = true;
  K.ctl = c.take<TokensCtl> (1);
  K.tile_count = c.take<long long> (K.n_tiles + 1);
  K.tile_begin = R.tile_begin = c.take<long long> (K.n_tiles + 1);
  R.cub = cub_room (c, 0, K.n_tiles + 1);
  return R;
}

/* a table keyword -> vocabulary id has an entry for every keyword the plan can report */
bool
tokens_table_covers (const ACMPlan *plan, const uint32_t *tok_of, uint64_t n_keywords) {
  return !tok_of || n_keywords >= plan->covered_keywords;
}

/* what every entry checks of the mode: SYMBOL reads the text as numbers of 1 or 2 bytes */
bool
tokens_mode_ok (uint32_t sym_bytes, uint32_t gap_base, uint32_t mode) {
  if (mode > ACM_TOKENS_GAP_DROP)
    return false;
  return mode != ACM_TOKENS_GAP_SYMBOL || (sym_bytes <= 2 && (uint64_t)gap_base <= (1ull << 32) - (1ull << (8 * sym_bytes)));
}

/* the passes over a selection of n records, or of *d_n in a room of n */
int
tokens_records (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const ACMRecord *d_sel, uint64_t n,
                const uint64_t *d_n, const uint64_t *d_offsets, uint64_t n_texts, const uint32_t *d_tok_of, uint64_t n_keywords, uint32_t gap_base,
                uint32_t mode, uint32_t *d_tok_id, uint64_t *d_tok_start, uint32_t *d_tok_len, uint64_t token_capacity, uint64_t *d_n_tokens,
                uint64_t *d_tok_first, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_n_tokens || !d_tmp || n >= (1ull << 31) || (n && !d_sel) || (!d_offsets && d_tok_first) || (d_offsets && n_texts >= (1ull << 31)) ||
      n_keywords >= (1ull << 32) || n_symbols >= (1ull << 56))
    return ACM_GPU_E_ARG;
  const uint32_t sb = plan->text_sym_bytes;
  if (!tokens_mode_ok (sb, gap_base, mode))
    return ACM_GPU_E_ARG;
  if (mode == ACM_TOKENS_GAP_SYMBOL && ((n_symbols && !d_text) || reinterpret_cast<uintptr_t> (d_text) % sb))
    return ACM_GPU_E_ARG;
  Carve carve (d_tmp);
  TokensK K{};
  const TokensRoom L = tokens_carve (carve, n_symbols, K);
  if (!L.ok || tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  K.sel = d_sel;
  K.capacity = n;
  K.n_dev = reinterpret_cast<const unsigned long long *> (d_n);
  K.text = static_cast<const unsigned char *> (d_text);
  K.n_symbols = n_symbols;
  K.pos_base = pos_base;
  K.sb = sb;
  K.mode = mode;
  K.gap_base = gap_base;
  K.offsets = reinterpret_cast<const unsigned long long *> (d_offsets);
  K.n_texts = d_offsets ? n_texts : 0;
  K.tok_of = d_tok_of;
  K.n_keywords = n_keywords;
  K.tok_id = d_tok_id;
  K.tok_start = reinterpret_cast<unsigned long long *> (d_tok_start);
  K.tok_len = d_tok_len;
  K.token_capacity = d_tok_id ? token_capacity : 0;
  K.d_n_tokens = reinterpret_cast<unsigned long long *> (d_n_tokens);
  K.tok_first = reinterpret_cast<unsigned long long *> (d_tok_first);
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (TokensCtl), st));
  /* a. the grid by the rooms the caller names */
  const uint64_t check_blocks = std::max ((n + TOKENS_THREADS - 1) / TOKENS_THREADS, d_offsets ? (n_texts + TOKENS_THREADS) / TOKENS_THREADS : (uint64_t)0);
  HIP_TRY (launch (tokens_check_kernel, capped_grid (plan, check_blocks), dim3 (TOKENS_THREADS), 0, st, K));
  /* b. c. d. the grid by the tiles of the text */
  HIP_TRY (launch (tokens_tile_kernel<false>, capped_grid (plan, K.n_tiles + 1), dim3 (TOKENS_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, K.tile_count, L.tile_begin, K.n_tiles + 1, st));
  HIP_TRY (launch (tokens_tile_kernel<true>, capped_grid (plan, std::max (K.n_tiles, d_offsets ? (n_texts + TOKENS_THREADS) / TOKENS_THREADS / 64 : (uint64_t)0)),
                   dim3 (TOKENS_THREADS), 0, st, K));
  return ACM_GPU_OK;
}
} // namespace

extern "C" size_t
acm_gpu_tokens_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_symbols) {
  if (!plan || n_or_capacity >= (1ull << 31))
    return 0;
  Carve c; /* (the passes keep nothing per record) */
  TokensK K{};
  return tokens_carve (c, n_symbols, K).ok ? c.total () : 0;
}

extern "C" int
acm_gpu_tokens_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const ACMRecord *d_sel, uint64_t n,
                               const uint64_t *d_n, const uint64_t *d_offsets, uint64_t n_texts, const uint32_t *d_tok_of, uint64_t n_keywords,
                               uint32_t gap_base, uint32_t mode, uint32_t *d_tok_id, uint64_t *d_tok_start, uint32_t *d_tok_len,
                               uint64_t token_capacity, uint64_t *d_n_tokens, uint64_t *d_tok_first, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || n_symbols >= (1ull << 56))
    return ACM_GPU_E_ARG;
  return tokens_records (plan, d_text, n_symbols, pos_base, d_sel, n, d_n, d_offsets, n_texts, d_tok_of, n_keywords, gap_base,
                         mode, d_tok_id, d_tok_start, d_tok_len, token_capacity, d_n_tokens, d_tok_first, d_tmp, tmp_bytes, stream);
}

extern "C" size_t
acm_gpu_scan_tokens_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || capacity >= (1ull << 31))
    return 0;
  /* (one room for both forms of the call: the scans and the selection have ended when the token passes begin) */
  const size_t scans = std::max (acm_gpu_scan_select_tmp_bytes (plan, capacity, n_symbols),
                                 std::max (acm_gpu_scan_batch_tmp_bytes (plan, capacity, n_symbols, n_texts), acm_gpu_select_tmp_bytes (plan, capacity, n_symbols)));
  return std::max (scans, acm_gpu_tokens_tmp_bytes (plan, capacity, n_symbols));
}

extern "C" int
acm_gpu_scan_tokens_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                            ACMRecord *d_records, uint64_t capacity, uint64_t *d_count, const uint32_t *d_tok_of, uint64_t n_keywords, uint32_t gap_base,
                            uint32_t mode, uint32_t *d_tok_id, uint64_t *d_tok_start, uint32_t *d_tok_len, uint64_t token_capacity,
                            uint64_t *d_n_tokens, uint64_t *d_tok_first, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || !d_n_tokens || !d_tmp || capacity >= (1ull << 31) || n_symbols >= (1ull << 56) || (n_symbols && !d_text) ||
      (capacity && !d_records) || (!d_offsets && d_tok_first) || (d_offsets && (pos_base || n_texts >= (1ull << 31))) ||
      !tokens_mode_ok (plan->text_sym_bytes, gap_base, mode) || !tokens_table_covers (plan, d_tok_of, n_keywords))
    return ACM_GPU_E_ARG;
  if (tmp_bytes < acm_gpu_scan_tokens_tmp_bytes (plan, capacity, n_symbols, n_texts))
    return ACM_GPU_E_ARG;
  int rc;
  if (!d_offsets)
    rc = acm_gpu_scan_select_device (plan, d_text, n_symbols, pos_base, d_records, capacity, d_count, d_tmp, tmp_bytes, stream);
  else {
    rc = acm_gpu_scan_batch_device (plan, d_text, n_symbols, d_offsets, n_texts, d_records, nullptr, nullptr, capacity, d_count, d_tmp, tmp_bytes, stream);
    if (!rc && capacity && n_symbols) /* (no room: *d_count says what the records need; no text: 0) */
      rc = acm_gpu_select_records_device (plan, d_records, capacity, d_count, 0, n_symbols, d_records, d_count, d_tmp, tmp_bytes, stream);
  }
  if (rc)
    return rc;
  return tokens_records (plan, d_text, n_symbols, pos_base, d_records, capacity, d_count, d_offsets, n_texts, d_tok_of, n_keywords, gap_base, mode,
                         d_tok_id, d_tok_start, d_tok_len, token_capacity, d_n_tokens, d_tok_first, d_tmp, tmp_bytes, stream);
}

extern "C" int
acm_gpu_scan_tokens_host (ACMPlan *plan, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const uint32_t *tok_of,
                          uint64_t n_keywords, uint32_t gap_base, uint32_t mode, uint32_t *tok_id, uint64_t *tok_start, uint32_t *tok_len,
                          uint64_t token_capacity, uint64_t *n_tokens, uint64_t *tok_first, uint64_t *n_selected) {
  if (!plan || !n_tokens || (n_symbols && !text) || (!offsets && tok_first) || n_keywords >= (1ull << 32) ||
      !tokens_mode_ok (plan->text_sym_bytes, gap_base, mode) || !tokens_table_covers (plan, tok_of, n_keywords) ||
      !optional_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_res = nullptr, *d_off = nullptr, *d_first = nullptr, *d_start = nullptr; /* d_res: the count, the tokens */
  uint32_t *d_of = nullptr, *d_id = nullptr, *d_len = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_res, 16));
  uint64_t matches = 0;
  int rc = count_first (plan, d_text, n_symbols, d_res, &matches);
  if (rc)
    return rc;
  if (offsets && matches == 0) /* (the batch scan is given room for a record) */
    matches = 1;
  const uint64_t room = tok_id ? token_capacity : 0;
  const size_t tmp_bytes = acm_gpu_scan_tokens_tmp_bytes (plan, matches, n_symbols, n_texts);
  HOST_TRY (temps.get (&d_rec, matches * 16));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  if (tok_id) {
    HOST_TRY (temps.get (&d_id, room * 4));
    if (tok_start)
      HOST_TRY (temps.get (&d_start, room * 8));
    if (tok_len)
      HOST_TRY (temps.get (&d_len, room * 4));
  }
  if (tok_of) {
    HOST_TRY (temps.get (&d_of, n_keywords * 4));
    if (n_keywords)
      HOST_TRY (hipMemcpy (d_of, tok_of, n_keywords * 4, hipMemcpyHostToDevice));
  }
  if (offsets) {
    HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
    if (tok_first)
      HOST_TRY (temps.get (&d_first, (n_texts + 1) * 8));
  }
  rc = settle (plan, acm_gpu_scan_tokens_device (plan, d_text, n_symbols, 0, d_off, n_texts, d_rec, matches, d_res, tok_of ? d_of : nullptr, n_keywords,
                                                 gap_base, mode, tok_id ? d_id : nullptr, d_start, d_len, room, d_res + 1, d_first, d_tmp, tmp_bytes,
                                                 nullptr), true);
  if (rc)
    return rc;
  uint64_t res[2] = { 0, 0 };
  HOST_TRY (hipMemcpy (res, d_res, 16, hipMemcpyDeviceToHost));
  if (res[0] > matches) /* (the scan found more than the count said: never expected) */
    return ACM_GPU_E_INTERNAL;
  *n_tokens = res[1];
  if (n_selected)
    *n_selected = res[0];
  if (tok_first)
    HOST_TRY (hipMemcpy (tok_first, d_first, (n_texts + 1) * 8, hipMemcpyDeviceToHost));
  if (!tok_id)
    return ACM_GPU_OK;
  if (res[1] > token_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (res[1]) {
    HOST_TRY (hipMemcpy (tok_id, d_id, (size_t)res[1] * 4, hipMemcpyDeviceToHost));
    if (tok_start)
      HOST_TRY (hipMemcpy (tok_start, d_start, (size_t)res[1] * 8, hipMemcpyDeviceToHost));
    if (tok_len)
      HOST_TRY (hipMemcpy (tok_len, d_len, (size_t)res[1] * 4, hipMemcpyDeviceToHost));
  }
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ whole-word matches (include/acm_gpu.h, dev_words.h)
 * One stable compaction of a record set under the symbols next to each match: the check of
 * offsets[], the mark pass, the prefix over the tiles, the write pass. */
namespace {
/* what words_carve derives beside K's pointers: the tile counts and their sums as the sum takes them */
struct WordsRoom {
  long long *count = nullptr, *begin = nullptr;
  CubRoom cub;
};
WordsRoom
words_carve (Carve &c, uint64_t capacity, WordsK &K) {
  WordsRoom R;
  /* ACM_GPU_WORDS_TILE=<records>: the passes' tile, a multiple of 64 (tests) */
  K.tile = tunable ("ACM_GPU_WORDS_TILE", WORDS_TILE_DEFAULT, WORDS_TILE_MIN, WORDS_TILE_MAX, Tune::MultWave);
  K.n_tiles = (capacity + K.tile - 1) / K.tile;
  K.ctl = c.take<WordsCtl> (1);
  R.count = c.take<long long> (K.n_tiles + 1);
  R.begin = c.take<long long> (K.n_tiles + 1);
  R.cub = cub_room (c, 0, K.n_tiles + 1);
  K.mask = c.take<unsigned long long> (((size_t)capacity + WAVE - 1) / WAVE);
  K.tile_count = reinterpret_cast<unsigned long long *> (R.count);
  K.tile_begin = reinterpret_cast<const unsigned long long *> (R.begin);
  return R;
}

/* the word set of a call into the kernels' arguments: the caller's symbols as unsigned integers */
bool
words_ranges (WordsK &K, uint32_t sb, const void *ranges, uint32_t n_ranges, uint32_t flags) {
  if (!acm_internal_words_args_ok (sb, ranges, n_ranges, flags))
    return false;
  for (uint32_t j = 0; j < n_ranges; j++) {
    unsigned long long lo = 0, hi = 0;
    memcpy (&lo, static_cast<const unsigned char *> (ranges) + (size_t)(2 * j) * sb, sb);
    memcpy (&hi, static_cast<const unsigned char *> (ranges) + (size_t)(2 * j + 1) * sb, sb);
    K.lo[j] = lo;
    K.hi[j] = hi;
  }
  K.n_ranges = n_ranges;
  K.flags = flags;
  return true;
}

template <int SB>
int
words_launch (const ACMPlan *plan, const WordsRoom &L, const WordsK &K, hipStream_t st) {
  HIP_TRY (launch (words_mark_kernel<SB>, capped_grid (plan, K.n_tiles + 1), dim3 (WORDS_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, L.count, L.begin, K.n_tiles + 1, st));
  HIP_TRY (launch (words_write_kernel, capped_grid (plan, K.n_tiles), dim3 (WORDS_THREADS), 0, st, K));
  return ACM_GPU_OK;
}
} // namespace

extern "C" size_t
acm_gpu_words_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: a record's text is a bisection of offsets[]) */
  if (!plan || n_or_capacity >= (1ull << 31))
    return 0;
  Carve c;
  WordsK K{};
  words_carve (c, n_or_capacity, K);
  return c.total ();
}

extern "C" int
acm_gpu_words_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                              const void *ranges, uint32_t n_ranges, uint32_t flags, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n,
                              ACMRecord *d_out, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || n >= (1ull << 31) || n_symbols >= (1ull << 56) || (n_symbols && !d_text) || (n && (!d_records || !d_out || !d_tmp)) ||
      (d_offsets && (n_texts >= (1ull << 31) || (n_texts == 0 && n_symbols))))
    return ACM_GPU_E_ARG;
  const uint32_t sb = plan->text_sym_bytes;
  WordsK K{};
  if (!words_ranges (K, sb, ranges, n_ranges, flags) || reinterpret_cast<uintptr_t> (d_text) % sb)
    return ACM_GPU_E_ARG;
  if (n) { /* (the output is written while the input is still read) */
    const uintptr_t a = reinterpret_cast<uintptr_t> (d_records), b = reinterpret_cast<uintptr_t> (d_out);
    if (a < b + n * sizeof (ACMRecord) && b < a + n * sizeof (ACMRecord))
      return ACM_GPU_E_ARG;
  }
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n == 0) /* (no room) */
    return no_record (plan, d_n, d_count, st);
  Carve carve (d_tmp);
  const WordsRoom L = words_carve (carve, n, K);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.text = static_cast<const unsigned char *> (d_text);
  K.n_symbols = n_symbols;
  K.pos_base = pos_base;
  K.offsets = n_texts ? d_offsets : nullptr; /* (no text: no symbol, every record breaks the contract) */
  K.n_texts = n_texts;
  K.in = d_records;
  K.capacity = n;
  K.n_dev = reinterpret_cast<const unsigned long long *> (d_n);
  K.out = d_out;
  K.d_count = reinterpret_cast<unsigned long long *> (d_count);
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (WordsCtl), st));
  if (K.offsets) /* one size, whatever the number of texts */
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + WORDS_THREADS - 1) / WORDS_THREADS), dim3 (WORDS_THREADS), 0, st, K.offsets, K.n_texts,
                     K.n_symbols, &K.ctl->bad, K.error));
  switch (sb) {
  case 1: return words_launch<1> (plan, L, K, st);
  case 2: return words_launch<2> (plan, L, K, st);
  case 4: return words_launch<4> (plan, L, K, st);
  case 8: return words_launch<8> (plan, L, K, st);
  default: return ACM_GPU_E_ARG;
  }
}

namespace {
/* the scratch of a fused call (scan_words, scan_patterns, scan_chains, scan_approx, ...): the ordered scan's records, then
 * the room the scan and the passes behind it share -- `passes_bytes` is what those report -- (the scan has ended when they
 * begin) */
struct ScanRoom {
  ACMRecord *found = nullptr;
  unsigned char *work = nullptr;
  size_t work_bytes = 0;
};
ScanRoom
scan_room_carve (Carve &c, const ACMPlan *plan, size_t passes_bytes, uint64_t capacity, uint64_t n_symbols) {
  ScanRoom R;
  R.work_bytes = std::max (acm_gpu_scan_ordered_tmp_bytes (plan, capacity, n_symbols), passes_bytes);
  R.found = c.take<ACMRecord> ((size_t)(capacity ? capacity : 1));
  R.work = c.take (R.work_bytes);
  return R;
}
} // namespace

extern "C" size_t
acm_gpu_scan_words_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || capacity >= (1ull << 31))
    return 0;
  Carve c;
  scan_room_carve (c, plan, acm_gpu_words_tmp_bytes (plan, capacity, n_texts), capacity, n_symbols);
  return c.total ();
}

extern "C" int
acm_gpu_scan_words_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                           const void *ranges, uint32_t n_ranges, uint32_t flags, ACMRecord *d_records, uint64_t capacity, uint64_t *d_count,
                           void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || capacity >= (1ull << 31) || (n_symbols && !d_text) || (capacity && (!d_records || !d_tmp)) ||
      !acm_internal_words_args_ok (plan->text_sym_bytes, ranges, n_ranges, flags))
    return ACM_GPU_E_ARG;
  Carve carve (capacity ? d_tmp : nullptr); /* (no room: nothing is bound) */
  const ScanRoom L = scan_room_carve (carve, plan, acm_gpu_words_tmp_bytes (plan, capacity, n_texts), capacity, n_symbols);
  if (capacity && tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  const int rc = acm_gpu_scan_ordered_device (plan, d_text, n_symbols, 0, pos_base, L.found, capacity, d_count, L.work, L.work_bytes, stream);
  if (rc || capacity == 0) /* (no room: *d_count says what the records need) */
    return rc;
  return acm_gpu_words_records_device (plan, d_text, n_symbols, pos_base, d_offsets, n_texts, ranges, n_ranges, flags, L.found, capacity, d_count,
                                       d_records, d_count, L.work, L.work_bytes, stream);
}

extern "C" int
acm_gpu_scan_words_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                         const void *ranges, uint32_t n_ranges, uint32_t flags, ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  if (!plan || !n_found || capacity >= (1ull << 31) || (n_symbols && !text) || (capacity && !records) ||
      !acm_internal_words_args_ok (plan->text_sym_bytes, ranges, n_ranges, flags) || !optional_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const size_t tmp_bytes = acm_gpu_scan_words_tmp_bytes (plan, capacity, n_symbols, n_texts);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_count = nullptr, *d_off = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_count, 8));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  if (offsets)
    HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  const int rc = acm_gpu_scan_words_device (plan, d_text, n_symbols, pos_base, d_off, n_texts, ranges, n_ranges, flags, d_rec, capacity, d_count, d_tmp,
                                            tmp_bytes, nullptr);
  return download_records (rc, d_count, d_rec, records, capacity, n_found);
}

/* ------------------------------------------------------------------ positions in code points and UTF-16 units (include/acm_chars.h, dev_chars.h)
 * The ruler: one pass over the text, two prefix sums over the tiles.  The maps: the check of offsets[], a lane per
 * record or position.  The plan gives its device, its caller symbol size (1) and its grid cap, nothing else. */
namespace {
/* where a ruler's arrays lie, for the most words a text of this size can touch (15 bytes off the grid); n_tiles is
 * that of the text's own address mod 16, `mis` */
struct CharsLayout {
  CharsHead H;
  uint64_t n_words = 0, most_tiles = 0;
  size_t bytes = 0;
};
CharsLayout
chars_layout (uint64_t n_symbols, uint32_t mis) {
  CharsLayout L;
  /* ACM_GPU_CHARS_TILE=<bytes of text>: the ruler pass's tile, a multiple of 256; ACM_GPU_CHARS_CHUNK=64, 128 or 256 (experiments) */
  uint32_t tile = tunable ("ACM_GPU_CHARS_TILE", CHARS_TILE_DEFAULT, CHARS_TILE_MIN, CHARS_TILE_MAX, Tune::Mult16);
  if (tile % 256)
    tile = CHARS_TILE_DEFAULT;
  const uint32_t chunk = tunable ("ACM_GPU_CHARS_CHUNK", CHARS_CHUNK_DEFAULT, CHARS_CHUNK_MIN, CHARS_CHUNK_MAX, Tune::Pow2);
  const uint64_t most_words = (n_symbols + 30) / 16;
  L.n_words = (n_symbols + mis + 15) / 16;
  L.most_tiles = (most_words * 16 + tile - 1) / tile;
  L.H = CharsHead{};
  L.H.magic = CHARS_MAGIC;
  L.H.chunk_log2 = chunk == 64 ? 6 : chunk == 128 ? 7 : 8;
  L.H.mis = mis;
  L.H.tile_words = tile / 16;
  L.H.n_symbols = n_symbols;
  L.H.n_tiles = (L.n_words * 16 + tile - 1) / tile;
  Carve c;
  c.take<CharsHead> (1);
  L.H.starts_at = c.boundary ();
  c.take<long long> (L.most_tiles + 1);
  L.H.wides_at = c.boundary ();
  c.take<long long> (L.most_tiles + 1);
  L.H.entry_at = c.boundary ();
  c.take<uint2> ((most_words * 16 + chunk - 1) / chunk + 1);
  L.bytes = c.total ();
  return L;
}

/* what the ruler pass derives beside the ruler: the tiles' totals as the sums take them, hipCUB's room */
struct CharsRulerRoom {
  long long *starts = nullptr, *wides = nullptr;
  CubRoom cub;
};
CharsRulerRoom
chars_ruler_carve (Carve &c, const CharsLayout &L) {
  CharsRulerRoom R;
  R.starts = c.take<long long> (L.most_tiles + 1);
  R.wides = c.take<long long> (L.most_tiles + 1);
  R.cub = cub_room (c, 0, L.most_tiles + 1);
  return R;
}

/* a byte plan and a text whose tiles the sums can count */
bool
chars_size_ok (const ACMPlan *plan, uint64_t n_symbols) {
  return plan && plan->text_sym_bytes == 1 && n_symbols < (1ull << 38);
}

bool
chars_unit_ok (uint32_t unit) {
  return unit == ACM_CHARS_CODEPOINTS || unit == ACM_CHARS_UTF16;
}

/* what the two maps share: the checks, the scratch, the check of offsets[] */
int
chars_map_begin (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint32_t unit, const void *d_ruler,
                 uint64_t n, void *d_tmp, size_t tmp_bytes, hipStream_t st, CharsMapK &K) {
  if (!chars_size_ok (plan, n_symbols) || !chars_unit_ok (unit) || n >= (1ull << 31) || (n_symbols && !d_text) || !d_ruler ||
      reinterpret_cast<uintptr_t> (d_ruler) % 16 || (n && !d_tmp) || (d_offsets && (n_texts >= (1ull << 31) || (n_texts == 0 && n_symbols))))
    return ACM_GPU_E_ARG;
  if (n == 0) /* (no room: nothing to write) */
    return ACM_GPU_OK;
  Carve carve (d_tmp);
  K.ctl = carve.take<CharsCtl> (1);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.text = static_cast<const unsigned char *> (d_text);
  K.n_symbols = n_symbols;
  K.mis = (uint32_t)(reinterpret_cast<uintptr_t> (d_text) & 15);
  K.utf16 = unit == ACM_CHARS_UTF16;
  K.offsets = n_texts ? d_offsets : nullptr; /* (no text: no symbol, one empty text) */
  K.n_texts = n_texts;
  K.ruler = static_cast<const unsigned char *> (d_ruler);
  K.capacity = n;
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (CharsCtl), st));
  if (K.offsets) /* one size, whatever the number of texts */
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + CHARS_THREADS - 1) / CHARS_THREADS), dim3 (CHARS_THREADS), 0, st, K.offsets, K.n_texts,
                     K.n_symbols, &K.ctl->bad, K.error));
  return ACM_GPU_OK;
}
} // namespace

extern "C" size_t
acm_gpu_chars_ruler_bytes (const ACMPlan *plan, uint64_t n_symbols) {
  return chars_size_ok (plan, n_symbols) ? chars_layout (n_symbols, 15).bytes : 0;
}

extern "C" size_t
acm_gpu_chars_ruler_tmp_bytes (const ACMPlan *plan, uint64_t n_symbols) {
  if (!chars_size_ok (plan, n_symbols))
    return 0;
  Carve c;
  chars_ruler_carve (c, chars_layout (n_symbols, 15));
  return c.total ();
}

extern "C" int
acm_gpu_chars_ruler_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, void *d_ruler, size_t ruler_bytes, void *d_tmp, size_t tmp_bytes,
                            void *stream) {
  if (!chars_size_ok (plan, n_symbols) || (n_symbols && !d_text) || !d_ruler || reinterpret_cast<uintptr_t> (d_ruler) % 16 || !d_tmp)
    return ACM_GPU_E_ARG;
  const CharsLayout L = chars_layout (n_symbols, (uint32_t)(reinterpret_cast<uintptr_t> (d_text) & 15));
  Carve carve (d_tmp);
  const CharsRulerRoom R = chars_ruler_carve (carve, L);
  if (ruler_bytes < L.bytes || tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  HIP_TRY (hipSetDevice (plan->device));
  unsigned char *ruler = static_cast<unsigned char *> (d_ruler);
  CharsRulerK K{};
  K.text = static_cast<const unsigned char *> (d_text);
  K.H = L.H;
  K.n_words = L.n_words;
  K.tile_starts = reinterpret_cast<unsigned long long *> (R.starts);
  K.tile_wides = reinterpret_cast<unsigned long long *> (R.wides);
  K.entry = reinterpret_cast<uint2 *> (ruler + L.H.entry_at);
  K.head = reinterpret_cast<CharsHead *> (ruler);
  HIP_TRY (launch (chars_ruler_kernel, capped_grid (plan, L.H.n_tiles + 1), dim3 (CHARS_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (R.cub, R.starts, reinterpret_cast<long long *> (ruler + L.H.starts_at), L.H.n_tiles + 1, st));
  HIP_TRY (exclusive_sum (R.cub, R.wides, reinterpret_cast<long long *> (ruler + L.H.wides_at), L.H.n_tiles + 1, st));
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_chars_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: a record's text is a bisection of offsets[]) */
  if (!plan || plan->text_sym_bytes != 1 || n_or_capacity >= (1ull << 31))
    return 0;
  Carve c;
  c.take<CharsCtl> (1);
  return c.total ();
}

extern "C" int
acm_gpu_chars_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                              uint32_t unit, const void *d_ruler, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, uint64_t *d_char_start,
                              uint32_t *d_char_len, uint8_t *d_edge, void *d_tmp, size_t tmp_bytes, void *stream) {
  if ((!d_char_start && !d_char_len && !d_edge) || (n && !d_records))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  CharsMapK K{};
  const int rc = chars_map_begin (plan, d_text, n_symbols, d_offsets, n_texts, unit, d_ruler, n, d_tmp, tmp_bytes, st, K);
  if (rc || n == 0) /* (no room: nothing to write) */
    return rc;
  K.pos_base = pos_base;
  K.in = d_records;
  K.n_dev = reinterpret_cast<const unsigned long long *> (d_n);
  K.char_start = reinterpret_cast<unsigned long long *> (d_char_start);
  K.char_len = d_char_len;
  K.edge = d_edge;
  HIP_TRY (launch (chars_records_kernel, capped_grid (plan, (n + CHARS_THREADS - 1) / CHARS_THREADS), dim3 (CHARS_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_chars_positions_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint32_t unit,
                                const void *d_ruler, const uint64_t *d_pos, uint64_t n, uint64_t *d_out, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (n && (!d_pos || !d_out))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  CharsMapK K{};
  const int rc = chars_map_begin (plan, d_text, n_symbols, d_offsets, n_texts, unit, d_ruler, n, d_tmp, tmp_bytes, st, K);
  if (rc || n == 0)
    return rc;
  K.pos = reinterpret_cast<const unsigned long long *> (d_pos);
  K.out = reinterpret_cast<unsigned long long *> (d_out);
  HIP_TRY (launch (chars_positions_kernel, capped_grid (plan, (n + CHARS_THREADS - 1) / CHARS_THREADS), dim3 (CHARS_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

namespace {
/* the scratch of acm_gpu_scan_chars_device: the ruler, then the room the scan, the ruler pass and the map share (each
 * has ended when the next begins) */
struct ScanCharsRoom {
  unsigned char *ruler = nullptr, *work = nullptr;
  size_t ruler_bytes = 0, work_bytes = 0;
};
ScanCharsRoom
scan_chars_carve (Carve &c, const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  ScanCharsRoom R;
  R.ruler_bytes = acm_gpu_chars_ruler_bytes (plan, n_symbols);
  R.work_bytes = std::max (acm_gpu_scan_ordered_tmp_bytes (plan, capacity, n_symbols),
                           std::max (acm_gpu_chars_ruler_tmp_bytes (plan, n_symbols), acm_gpu_chars_tmp_bytes (plan, capacity, n_texts)));
  R.ruler = c.take (R.ruler_bytes);
  R.work = c.take (R.work_bytes);
  return R;
}
} // namespace

extern "C" size_t
acm_gpu_scan_chars_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!chars_size_ok (plan, n_symbols) || capacity >= (1ull << 31))
    return 0;
  Carve c;
  scan_chars_carve (c, plan, capacity, n_symbols, n_texts);
  return c.total ();
}

extern "C" int
acm_gpu_scan_chars_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                           uint32_t unit, ACMRecord *d_records, uint64_t *d_char_start, uint32_t *d_char_len, uint8_t *d_edge, uint64_t capacity,
                           uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!chars_size_ok (plan, n_symbols) || !chars_unit_ok (unit) || !d_count || capacity >= (1ull << 31) || (n_symbols && !d_text) ||
      (capacity && (!d_records || !d_tmp)) || (!d_char_start && !d_char_len && !d_edge))
    return ACM_GPU_E_ARG;
  Carve carve (capacity ? d_tmp : nullptr); /* (no room: nothing is bound) */
  const ScanCharsRoom L = scan_chars_carve (carve, plan, capacity, n_symbols, n_texts);
  if (capacity && tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  int rc = acm_gpu_scan_ordered_device (plan, d_text, n_symbols, 0, pos_base, d_records, capacity, d_count, L.work, L.work_bytes, stream);
  if (rc || capacity == 0) /* (no room: *d_count says what the records need) */
    return rc;
  rc = acm_gpu_chars_ruler_device (plan, d_text, n_symbols, L.ruler, L.ruler_bytes, L.work, L.work_bytes, stream);
  if (rc)
    return rc;
  return acm_gpu_chars_records_device (plan, d_text, n_symbols, pos_base, d_offsets, n_texts, unit, L.ruler, d_records, capacity, d_count, d_char_start,
                                       d_char_len, d_edge, L.work, L.work_bytes, stream);
}

extern "C" int
acm_gpu_scan_chars_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts, uint32_t unit,
                         ACMRecord *records, uint64_t *char_start, uint32_t *char_len, uint8_t *edge, uint64_t capacity, uint64_t *n_found) {
  if (!chars_size_ok (plan, n_symbols) || !chars_unit_ok (unit) || !n_found || capacity >= (1ull << 31) || (n_symbols && !text) ||
      (capacity && !records) || (!char_start && !char_len && !edge) || !optional_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const size_t tmp_bytes = acm_gpu_scan_chars_tmp_bytes (plan, capacity, n_symbols, n_texts);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_count = nullptr, *d_off = nullptr, *d_start = nullptr;
  uint32_t *d_len = nullptr;
  uint8_t *d_edge = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_count, 8));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  HOST_TRY (temps.get (&d_start, capacity * 8));
  HOST_TRY (temps.get (&d_len, capacity * 4));
  HOST_TRY (temps.get (&d_edge, capacity));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  if (offsets)
    HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  int rc = acm_gpu_scan_chars_device (plan, d_text, n_symbols, pos_base, d_off, n_texts, unit, d_rec, d_start, d_len, d_edge, capacity, d_count, d_tmp,
                                      tmp_bytes, nullptr);
  rc = download_records (rc, d_count, d_rec, records, capacity, n_found);
  if (rc || *n_found == 0)
    return rc;
  if (char_start)
    HOST_TRY (hipMemcpy (char_start, d_start, *n_found * 8, hipMemcpyDeviceToHost));
  if (char_len)
    HOST_TRY (hipMemcpy (char_len, d_len, *n_found * 4, hipMemcpyDeviceToHost));
  if (edge)
    HOST_TRY (hipMemcpy (edge, d_edge, *n_found, hipMemcpyDeviceToHost));
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ match contexts (include/acm_gpu.h, dev_context.h)
 * Records into windows, windows into snippets, snippets into one packed output: the check of
 * offsets[], the window pass, under MERGE the carries over the tiles and the flag pass, the prefix
 * sums over the tiles, the index pass and the gather. */
namespace {
/* what context_carve derives beside K's pointers: hipCUB's room */
struct ContextRoom {
  long long *cnt_begin = nullptr, *sum_begin = nullptr;
  CubRoom cub;
};
ContextRoom
context_carve (Carve &c, uint64_t capacity, ContextK &K) {
  ContextRoom R;
  /* ACM_GPU_CONTEXT_TILE=<records>: the passes' tile, a multiple of 64 (tests) */
  K.tile = tunable ("ACM_GPU_CONTEXT_TILE", CONTEXT_TILE_DEFAULT, CONTEXT_TILE_MIN, CONTEXT_TILE_MAX, Tune::MultWave);
  K.n_tiles = (capacity + K.tile - 1) / K.tile;
  K.ctl = c.take<ContextCtl> (1);
  K.tile_lo = c.take<unsigned long long> (K.n_tiles + 1);
  K.tile_hi = c.take<unsigned long long> (K.n_tiles + 1);
  K.tile_cnt = c.take<long long> (K.n_tiles + 1);
  K.tile_sum = c.take<long long> (K.n_tiles + 1);
  K.tile_cnt_begin = R.cnt_begin = c.take<long long> (K.n_tiles + 1);
  K.tile_sum_begin = R.sum_begin = c.take<long long> (K.n_tiles + 1);
  R.cub = cub_room (c, 0, K.n_tiles + 1);
  K.lo = c.take<unsigned long long> ((size_t)capacity);
  K.hi = c.take<unsigned long long> ((size_t)capacity);
  K.tx = c.take<uint32_t> ((size_t)capacity);
  return R;
}

/* CONTEXT's flags on the device: the two bits, TEXTS only over offsets[] */
bool
context_flags_ok (uint32_t flags, const uint64_t *offsets) {
  return flags <= (ACM_CONTEXT_TEXTS | ACM_CONTEXT_MERGE) && (!(flags & ACM_CONTEXT_TEXTS) || offsets);
}
} // namespace

extern "C" size_t
acm_gpu_context_tmp_bytes (const ACMPlan *plan, uint64_t n_or_capacity, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: a record's text is a bisection of offsets[]) */
  if (!plan || n_or_capacity >= (1ull << 31))
    return 0;
  Carve c;
  ContextK K{};
  context_carve (c, n_or_capacity, K);
  return c.total ();
}

extern "C" int
acm_gpu_context_records_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                                const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, uint32_t before, uint32_t after, uint32_t flags,
                                void *d_out, uint64_t out_capacity, uint64_t *d_out_symbols, uint64_t *d_n_snippets, uint64_t *d_snip_lo,
                                uint64_t *d_out_offsets, uint32_t *d_snip_text, uint32_t *d_rec_snip, int64_t *d_rec_at, void *d_tmp, size_t tmp_bytes,
                                void *stream) {
  if (!plan || !d_out_symbols || !d_n_snippets || !d_out_offsets || n >= (1ull << 31) || (n_symbols && !d_text) ||
      (n && (!d_records || !d_snip_lo || !d_tmp)) || !context_flags_ok (flags, d_offsets) ||
      (d_offsets && (n_texts >= (1ull << 31) || (n_texts == 0 && n_symbols))))
    return ACM_GPU_E_ARG;
  const uint32_t sb = plan->text_sym_bytes;
  if (!symbols_ok (d_text, n_symbols, sb) || (d_out && (!symbols_ok (d_out, out_capacity, sb) || !apart (d_text, n_symbols, d_out, out_capacity, sb))))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n == 0) { /* (no room: no snippet; a count that came in above 0 is an overflow, which reports the same) */
    HIP_TRY (hipMemsetAsync (d_n_snippets, 0, 8, st));
    HIP_TRY (hipMemsetAsync (d_out_symbols, 0, 8, st));
    HIP_TRY (hipMemsetAsync (d_out_offsets, 0, 8, st));
    return ACM_GPU_OK;
  }
  Carve carve (d_tmp);
  ContextK K{};
  const ContextRoom L = context_carve (carve, n, K);
  if (tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  K.text = static_cast<const unsigned char *> (d_text);
  K.n_symbols = n_symbols;
  K.pos_base = pos_base;
  K.offsets = n_texts ? d_offsets : nullptr; /* (no text: no symbol, every record breaks the contract) */
  K.n_texts = n_texts;
  K.in = d_records;
  K.capacity = n;
  K.n_dev = reinterpret_cast<const unsigned long long *> (d_n);
  K.before = before;
  K.after = after;
  K.flags = flags;
  K.d_n_snippets = reinterpret_cast<unsigned long long *> (d_n_snippets);
  K.d_out_symbols = reinterpret_cast<unsigned long long *> (d_out_symbols);
  K.d_snip_lo = reinterpret_cast<unsigned long long *> (d_snip_lo);
  K.d_out_offsets = reinterpret_cast<long long *> (d_out_offsets);
  K.d_snip_text = d_snip_text;
  K.d_rec_snip = d_rec_snip;
  K.d_rec_at = reinterpret_cast<long long *> (d_rec_at);
  K.out = static_cast<unsigned char *> (d_out);
  K.out_capacity = out_capacity;
  K.sb = sb;
  /* ACM_GPU_CONTEXT_OUT_TILE=<bytes of output>: the gather's tile, a multiple of 16 (tests) */
  K.tile_words = tunable ("ACM_GPU_CONTEXT_OUT_TILE", CONTEXT_OUT_TILE_DEFAULT, CONTEXT_OUT_TILE_MIN, CONTEXT_OUT_TILE_MAX, Tune::Mult16) / 16;
  K.error = error_word (plan);
  const bool merge = (flags & ACM_CONTEXT_MERGE) != 0;
  const dim3 block (CONTEXT_THREADS), tiles_grid = capped_grid (plan, K.n_tiles + 1);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (ContextCtl), st));
  if (K.offsets) /* one size, whatever the number of texts */
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + CONTEXT_THREADS - 1) / CONTEXT_THREADS), block, 0, st, K.offsets, K.n_texts, K.n_symbols,
                     &K.ctl->bad, K.error));
  /* 1. */
  HIP_TRY (merge ? launch (context_window_kernel<true>, tiles_grid, block, 0, st, K) : launch (context_window_kernel<false>, tiles_grid, block, 0, st, K));
  if (merge) { /* 2., 3. */
    HIP_TRY (launch (context_carry_kernel, dim3 (1), block, 0, st, K));
    HIP_TRY (launch (context_flag_kernel, tiles_grid, block, 0, st, K));
    HIP_TRY (exclusive_sum (L.cub, K.tile_cnt, L.cnt_begin, K.n_tiles + 1, st));
  }
  /* 4. */
  HIP_TRY (exclusive_sum (L.cub, K.tile_sum, L.sum_begin, K.n_tiles + 1, st));
  HIP_TRY (merge ? launch (context_index_kernel<true>, tiles_grid, block, 0, st, K) : launch (context_index_kernel<false>, tiles_grid, block, 0, st, K));
  /* 5. the grid by the room of the output, not by what the passes found */
  if (d_out && out_capacity)
    HIP_TRY (launch (context_gather_kernel, capped_grid (plan, (out_capacity * sb + 15 + 16) / ((uint64_t)K.tile_words * 16) + 1), block, 0, st, K));
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_scan_context_tmp_bytes (const ACMPlan *plan, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || capacity >= (1ull << 31))
    return 0;
  /* (the scan has ended when the context passes begin: they read d_records) */
  return std::max (acm_gpu_scan_ordered_tmp_bytes (plan, capacity, n_symbols), acm_gpu_context_tmp_bytes (plan, capacity, n_texts));
}

extern "C" int
acm_gpu_scan_context_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts,
                             ACMRecord *d_records, uint64_t capacity, uint64_t *d_count, uint32_t before, uint32_t after, uint32_t flags, void *d_out,
                             uint64_t out_capacity, uint64_t *d_out_symbols, uint64_t *d_n_snippets, uint64_t *d_snip_lo, uint64_t *d_out_offsets,
                             uint32_t *d_snip_text, uint32_t *d_rec_snip, int64_t *d_rec_at, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || !d_out_symbols || !d_n_snippets || !d_out_offsets || capacity >= (1ull << 31) || (n_symbols && !d_text) ||
      (capacity && (!d_records || !d_snip_lo || !d_tmp)) || !context_flags_ok (flags, d_offsets) ||
      (d_offsets && (n_texts >= (1ull << 31) || (n_texts == 0 && n_symbols))))
    return ACM_GPU_E_ARG;
  if (d_out && (!symbols_ok (d_out, out_capacity, plan->text_sym_bytes) || !apart (d_text, n_symbols, d_out, out_capacity, plan->text_sym_bytes)))
    return ACM_GPU_E_ARG; /* (refused before the scan runs, not behind it) */
  if (capacity && tmp_bytes < acm_gpu_scan_context_tmp_bytes (plan, capacity, n_symbols, n_texts))
    return ACM_GPU_E_ARG;
  const int rc = acm_gpu_scan_ordered_device (plan, d_text, n_symbols, 0, pos_base, d_records, capacity, d_count, d_tmp, tmp_bytes, stream);
  if (rc)
    return rc;
  return acm_gpu_context_records_device (plan, d_text, n_symbols, pos_base, d_offsets, n_texts, d_records, capacity, d_count, before, after, flags, d_out,
                                         out_capacity, d_out_symbols, d_n_snippets, d_snip_lo, d_out_offsets, d_snip_text, d_rec_snip, d_rec_at, d_tmp,
                                         tmp_bytes, stream);
}

extern "C" int
acm_gpu_scan_context_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                           ACMRecord *records, uint64_t capacity, uint64_t *n_found, uint32_t before, uint32_t after, uint32_t flags, void *out,
                           uint64_t out_capacity, uint64_t *out_symbols, uint64_t *n_snippets, uint64_t *snip_lo, uint64_t *out_offsets,
                           uint32_t *snip_text, uint32_t *rec_snip, int64_t *rec_at) {
  if (!plan || !n_found || !out_symbols || !n_snippets || capacity >= (1ull << 31) || (n_symbols && !text) || (out_capacity && !out) ||
      !context_flags_ok (flags, offsets) || !optional_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const uint32_t sb = plan->text_sym_bytes;
  const size_t tmp_bytes = acm_gpu_scan_context_tmp_bytes (plan, capacity, n_symbols, n_texts);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr, *d_out = nullptr;
  uint64_t *d_res = nullptr, *d_off = nullptr, *d_lo = nullptr, *d_oo = nullptr; /* d_res: the count, the snippets, the output's symbols */
  uint32_t *d_st = nullptr, *d_rs = nullptr;
  int64_t *d_ra = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (temps.get (&d_res, 24));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  HOST_TRY (temps.get (&d_lo, capacity * 8));
  HOST_TRY (temps.get (&d_oo, (capacity + 1) * 8));
  if (snip_text)
    HOST_TRY (temps.get (&d_st, capacity * 4));
  if (rec_snip)
    HOST_TRY (temps.get (&d_rs, capacity * 4));
  if (rec_at)
    HOST_TRY (temps.get (&d_ra, capacity * 8));
  if (out)
    HOST_TRY (temps.get (&d_out, (size_t)out_capacity * sb));
  if (offsets)
    HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  const int rc = settle (plan, acm_gpu_scan_context_device (plan, d_text, n_symbols, pos_base, d_off, n_texts, d_rec, capacity, d_res, before, after, flags,
                                                            d_out, out_capacity, d_res + 2, d_res + 1, d_lo, d_oo, d_st, d_rs, d_ra, d_tmp, tmp_bytes, nullptr),
                         true);
  if (rc)
    return rc;
  uint64_t res[3] = { 0, 0, 0 };
  HOST_TRY (hipMemcpy (res, d_res, 24, hipMemcpyDeviceToHost));
  *n_found = res[0];
  if (res[0] > capacity) /* the first meaning: only *n_found is valid */
    return ACM_GPU_E_OVERFLOW;
  *n_snippets = res[1];
  *out_symbols = res[2];
  if (records && res[0])
    HOST_TRY (hipMemcpy (records, d_rec, res[0] * 16, hipMemcpyDeviceToHost));
  if (snip_lo && res[1])
    HOST_TRY (hipMemcpy (snip_lo, d_lo, res[1] * 8, hipMemcpyDeviceToHost));
  if (out_offsets)
    HOST_TRY (hipMemcpy (out_offsets, d_oo, (res[1] + 1) * 8, hipMemcpyDeviceToHost));
  if (snip_text && res[1])
    HOST_TRY (hipMemcpy (snip_text, d_st, res[1] * 4, hipMemcpyDeviceToHost));
  if (rec_snip && res[0])
    HOST_TRY (hipMemcpy (rec_snip, d_rs, res[0] * 4, hipMemcpyDeviceToHost));
  if (rec_at && res[0])
    HOST_TRY (hipMemcpy (rec_at, d_ra, res[0] * 8, hipMemcpyDeviceToHost));
  if (out && res[2] > out_capacity) /* the second: everything but `out` is valid */
    return ACM_GPU_E_OVERFLOW;
  if (out && res[2])
    HOST_TRY (hipMemcpy (out, d_out, (size_t)res[2] * sb, hipMemcpyDeviceToHost));
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ anchored matches and dictionary lookup (include/acm_gpu.h, dev_anchored.h)
 * No scan: the check of offsets[], one lane per text walking the goto function from the root, and for
 * the records a prefix sum over the texts' counts and a second walk that writes them. */
namespace {
/* what anchored_carve derives beside K's pointers: the counts and their sums as the sum takes them */
struct AnchoredRoom {
  long long *count = nullptr, *first = nullptr;
  CubRoom cub;
};
AnchoredRoom
anchored_carve (Carve &c, uint64_t n_texts, bool records, AnchoredK &K) {
  AnchoredRoom R;
  K.ctl = c.take<AnchoredCtl> (1);
  if (!records) /* the lookup call: the count pass writes the caller's arrays and nothing else */
    return R;
  R.count = c.take<long long> (n_texts + 1);
  R.first = c.take<long long> (n_texts + 1);
  R.cub = cub_room (c, 0, n_texts + 1);
  K.count = reinterpret_cast<unsigned long long *> (R.count);
  K.first = reinterpret_cast<const unsigned long long *> (R.first);
  return R;
}

/* the plan's own trie is walked in the start-parallel tables: what acm_gpu_plan_update edits in place */
bool
anchored_in_starts (const ACMPlan *p) {
  return p->kind == PlanKind::Starts && p->mir != nullptr;
}

/* a plan's trie as the walk reads it, behind starts_flush and prepare_text (which set what is bound here) */
AnchoredTrie
anchored_trie (const ACMPlan *p, bool starts, const void *walked_text) {
  AnchoredTrie T{};
  if (starts) {
    T.starts.srec = p->TK.srec;
    T.starts.sedge = p->TK.sedge;
    T.starts.lut = p->TK.lut;
    T.lut_size = p->TK.lut_size;
  } else {
    T.csr.row_ptr = p->csr.row_ptr;
    T.csr.edge_sym = p->csr.edge_sym;
    T.csr.edge_next = p->csr.edge_next;
  }
  T.live = p->finfo.n_edges != 0 ? 1u : 0u;
  T.oinfo = p->d_oinfo;
  T.text = static_cast<const unsigned char *> (walked_text);
  return T;
}

/* pending updates of a start-parallel plan into its tables, then the text as the plan's kernels read it */
int
anchored_prepare (ACMPlan *p, const void **text, uint64_t n_symbols, hipStream_t st) {
  if (p->mir && (p->mir->full_upload || !p->mir->patches.empty ()))
    if (const int rc = starts_flush (p, st))
      return rc;
  /* the text as the plan compares it: interned ids, class ids (prepare_text; the host round of 4-byte class plans
   * included).  The aligned copy prepare_text makes for the scan kernels of other plans is not needed: the walk
   * takes one naturally aligned symbol at a time and would pay for the whole buffer to read lmax symbols a text */
  const bool mapped = p->d_intern || p->cls32 || p->d_classlut;
  return n_symbols && mapped ? prepare_text (p, text, n_symbols, st) : (int)ACM_GPU_OK;
}

template <int SB, bool STARTS>
int
anchored_passes (const ACMPlan *plan, const AnchoredRoom &L, const AnchoredK &K, hipStream_t st) {
  /* ACM_GPU_ANCHORED_GRID=<blocks>: the most blocks of the two passes (tests) */
  const uint32_t most = tunable ("ACM_GPU_ANCHORED_GRID", ANCHORED_GRID_MAX, 1, ANCHORED_GRID_MAX, Tune::Any);
  dim3 grid = capped_grid (plan, (K.n_texts + 1 + ANCHORED_THREADS - 1) / ANCHORED_THREADS);
  grid.x = std::min (grid.x, most);
  HIP_TRY (launch (anchored_count_kernel<SB, STARTS>, grid, dim3 (ANCHORED_THREADS), 0, st, K));
  if (!K.mode)
    return ACM_GPU_OK;
  HIP_TRY (exclusive_sum (L.cub, L.count, L.first, K.n_texts + 1, st));
  HIP_TRY (launch (anchored_fill_kernel<SB, STARTS>, grid, dim3 (ANCHORED_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

template <int SB>
int
anchored_launch (const ACMPlan *plan, const AnchoredRoom &L, const AnchoredK &K, hipStream_t st) {
  return anchored_in_starts (plan) ? anchored_passes<SB, true> (plan, L, K, st) : anchored_passes<SB, false> (plan, L, K, st);
}

/* both device calls behind their own argument checks; K: the outputs and the mode (0: lookup) */
int
anchored_call (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, AnchoredK &K, void *d_tmp,
               size_t tmp_bytes, hipStream_t st) {
  Carve carve (d_tmp);
  const AnchoredRoom L = anchored_carve (carve, n_texts, K.mode != 0, K);
  if (!d_offsets || !d_tmp || tmp_bytes < carve.total () || (n_symbols && !d_text) || !symbols_ok (d_text, n_symbols, plan->text_sym_bytes))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  if (const int rc = mark_retired (plan, st))
    return rc;
  const void *text = d_text, *delta_text = d_text;
  if (const int rc = anchored_prepare (plan, &text, n_symbols, st))
    return rc;
  K.base = anchored_trie (plan, anchored_in_starts (plan), text);
  K.lmax = plan_lmax (plan);
  if (plan->delta) {
    if (const int rc = anchored_prepare (plan->delta, &delta_text, n_symbols, st))
      return rc;
    K.delta = anchored_trie (plan->delta, false, delta_text); /* (never edited in place: its CSR rows) */
  } else
    K.delta.text = K.base.text; /* (never read: the delta is not live) */
  K.offsets = reinterpret_cast<const unsigned long long *> (d_offsets);
  K.n_texts = n_texts;
  K.n_symbols = n_symbols;
  K.error = error_word (plan);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (AnchoredCtl), st));
  HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + ANCHORED_THREADS - 1) / ANCHORED_THREADS), dim3 (ANCHORED_THREADS), 0, st,
                   reinterpret_cast<const uint64_t *> (K.offsets), K.n_texts, K.n_symbols, &K.ctl->bad, K.error));
  switch (plan->finfo.sym_bytes) { /* (what the kernels walk: an interned 8-byte plan walks 4-byte ids) */
  case 1: return anchored_launch<1> (plan, L, K, st);
  case 2: return anchored_launch<2> (plan, L, K, st);
  case 4: return anchored_launch<4> (plan, L, K, st);
  default: return ACM_GPU_E_ARG;
  }
}

bool
anchored_mode_ok (uint32_t mode) {
  return mode >= ACM_ANCHORED_PREFIXES && mode <= ACM_ANCHORED_WHOLE;
}
} // namespace

extern "C" size_t
acm_gpu_scan_anchored_tmp_bytes (const ACMPlan *plan, uint64_t n_texts) {
  if (!plan || n_texts >= ANCHORED_MOST_TEXTS)
    return 0;
  Carve c;
  AnchoredK K{};
  anchored_carve (c, n_texts, true, K);
  return c.total ();
}

extern "C" size_t
acm_gpu_lookup_tmp_bytes (const ACMPlan *plan, uint64_t n_texts) {
  if (!plan || n_texts >= (1ull << 32))
    return 0;
  Carve c;
  AnchoredK K{};
  anchored_carve (c, n_texts, false, K);
  return c.total ();
}

extern "C" int
acm_gpu_scan_anchored_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint32_t mode,
                              ACMRecord *d_records, uint32_t *d_text_id, uint64_t *d_first, uint64_t capacity, uint64_t *d_count, void *d_tmp,
                              size_t tmp_bytes, void *stream) {
  if (!plan || !d_count || !anchored_mode_ok (mode) || n_texts >= ANCHORED_MOST_TEXTS || (capacity && !d_records))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0)
    return empty_batch (plan, n_symbols, { d_count, d_first }, st);
  AnchoredK K{};
  K.mode = mode;
  K.records = d_records;
  K.text_id = d_text_id;
  K.d_first = reinterpret_cast<unsigned long long *> (d_first);
  K.capacity = capacity;
  K.d_count = reinterpret_cast<unsigned long long *> (d_count);
  return anchored_call (plan, d_text, n_symbols, d_offsets, n_texts, K, d_tmp, tmp_bytes, st);
}

extern "C" int
acm_gpu_lookup_device (ACMPlan *plan, const void *d_text, uint64_t n_symbols, const uint64_t *d_offsets, uint64_t n_texts, uint32_t *d_whole_id,
                       uint32_t *d_prefix_id, uint32_t *d_prefix_len, void *d_tmp, size_t tmp_bytes, void *stream) {
  if (!plan || (!d_whole_id && !d_prefix_id && !d_prefix_len) || n_texts >= (1ull << 32))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n_texts == 0)
    return empty_batch (plan, n_symbols, {}, st);
  AnchoredK K{};
  K.whole_id = d_whole_id;
  K.prefix_id = d_prefix_id;
  K.prefix_len = d_prefix_len;
  return anchored_call (plan, d_text, n_symbols, d_offsets, n_texts, K, d_tmp, tmp_bytes, st);
}

extern "C" int
acm_gpu_scan_anchored_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t mode, ACMRecord *records,
                            uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  if (!plan || !n_found || !anchored_mode_ok (mode) || (capacity && !records) || !batch_args_ok (text, offsets, n_texts, ANCHORED_MOST_TEXTS))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const uint64_t n_symbols = offsets[n_texts];
  const size_t tmp_bytes = acm_gpu_scan_anchored_tmp_bytes (plan, n_texts);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_off = nullptr, *d_count = nullptr, *d_first = nullptr;
  uint32_t *d_tid = nullptr;
  ACMRecord *d_rec = nullptr;
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  HOST_TRY (temps.get (&d_count, 8));
  HOST_TRY (temps.get (&d_rec, capacity * 16));
  HOST_TRY (temps.get (&d_tid, capacity * 4));
  HOST_TRY (temps.get (&d_first, (n_texts + 1) * 8));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  const int rc = acm_gpu_scan_anchored_device (plan, d_text, n_symbols, d_off, n_texts, mode, d_rec, d_tid, d_first, capacity, d_count, d_tmp, tmp_bytes,
                                               nullptr);
  const BatchDownload down = { text_id, d_tid, first, d_first, n_texts, true };
  return download_records (rc, d_count, d_rec, records, capacity, n_found, &down);
}

extern "C" int
acm_gpu_lookup_host (ACMPlan *plan, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t *whole_id, uint32_t *prefix_id,
                     uint32_t *prefix_len) {
  if (!plan || (!whole_id && !prefix_id && !prefix_len) || !batch_args_ok (text, offsets, n_texts, 1ull << 32))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const uint64_t n_symbols = offsets[n_texts];
  const size_t tmp_bytes = acm_gpu_lookup_tmp_bytes (plan, n_texts);
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_off = nullptr;
  uint32_t *host[3] = { whole_id, prefix_id, prefix_len }, *dev[3] = { nullptr, nullptr, nullptr };
  HOST_TRY (upload_text (temps, plan, text, n_symbols, &d_text));
  HOST_TRY (upload_offsets (temps, offsets, n_texts, &d_off));
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  for (int a = 0; a < 3; a++)
    if (host[a])
      HOST_TRY (temps.get (&dev[a], n_texts * 4));
  if (const int rc = settle (plan, acm_gpu_lookup_device (plan, d_text, n_symbols, d_off, n_texts, dev[0], dev[1], dev[2], d_tmp, tmp_bytes, nullptr), false))
    return rc;
  for (int a = 0; a < 3; a++)
    if (host[a] && n_texts)
      HOST_TRY (hipMemcpy (host[a], dev[a], n_texts * 4, hipMemcpyDeviceToHost));
  HOST_TRY (hipDeviceSynchronize ());
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ the joins of a record set under a compiled set
 * PATTERNS, CHAINS and APPROX / EDIT / TEMPLATES (the sections below) are one frame around different passes: a
 * *_records_device call over JoinK (dev_all.h), a fused call that scans first, and a host form of the fused call.
 * What the three share, one copy of each. */
namespace {
/* the arguments every *_records_device of a join has, under their names in include/acm_gpu.h */
struct JoinCall {
  ACMPlan *plan;
  const ACMRecord *d_records;
  uint64_t n;
  const uint64_t *d_n;
  uint64_t n_symbols, pos_base;
  const uint64_t *d_offsets;
  uint64_t n_texts;
  ACMRecord *d_out;
  uint64_t out_capacity;
  uint64_t *d_count;
  void *d_tmp;
  size_t tmp_bytes;
  void *stream;
};

/* whether a join takes them with this set; the output is written while the input is still read, so the two lie apart */
bool
join_args_ok (const JoinCall &C, const DeviceSet *set) {
  return C.plan && set && set->device == C.plan->device && C.d_count && C.n < (1ull << 31) && C.out_capacity < (1ull << 31) &&
         C.n_symbols < (1ull << 56) && (!C.out_capacity || C.d_out) && (!C.n || (C.d_records && C.d_tmp)) &&
         (!C.d_offsets || (C.n_texts < (1ull << 31) && (C.n_texts || !C.n_symbols))) &&
         apart (C.d_records, C.n, C.d_out, C.out_capacity, sizeof (ACMRecord));
}

/* the head of a join's scratch and what the sum takes of it: tile geometry and control words first (a family may
 * take room of its own behind them), then the counts, their sums and hipCUB's room */
struct JoinRoom {
  long long *count = nullptr, *first = nullptr;
  CubRoom cub;
};
void
join_carve_ctl (Carve &c, uint64_t capacity, uint32_t tile, JoinK &K) {
  K.tile = tile;
  K.n_tiles = (capacity + tile - 1) / tile;
  K.ctl = c.take<JoinCtl> (1);
}
JoinRoom
join_carve_counts (Carve &c, uint64_t capacity, JoinK &K) {
  JoinRoom R;
  R.count = c.take<long long> ((size_t)capacity + 1);
  R.first = c.take<long long> ((size_t)capacity + 1);
  R.cub = cub_room (c, 0, capacity + 1);
  K.count = reinterpret_cast<unsigned long long *> (R.count);
  K.first = reinterpret_cast<const unsigned long long *> (R.first);
  return R;
}

/* the head of a join's kernel arguments from the call's */
void
bind_join (JoinK &K, const JoinCall &C) {
  K.in = C.d_records;
  K.capacity = C.n;
  K.n_dev = reinterpret_cast<const unsigned long long *> (C.d_n);
  K.n_symbols = C.n_symbols;
  K.pos_base = C.pos_base;
  K.offsets = C.n_texts ? C.d_offsets : nullptr; /* (no text: no symbol, every record breaks the contract) */
  K.n_texts = C.n_texts;
  K.out = C.d_out;
  K.out_capacity = C.out_capacity;
  K.d_count = reinterpret_cast<unsigned long long *> (C.d_count);
  K.error = error_word (C.plan);
}

/* the arguments every acm_gpu_scan_<join>_device has */
struct ScanJoinCall {
  ACMPlan *plan;
  const void *d_text;
  uint64_t n_symbols, pos_base;
  const uint64_t *d_offsets;
  uint64_t n_texts, capacity;
  ACMRecord *d_out;
  uint64_t out_capacity;
  uint64_t *d_count, *d_found;
  void *d_tmp;
  size_t tmp_bytes;
  void *stream;
};

/* A fused call: the ordered scan into `capacity` records of the call's own, then the family's join of them -- join
 * (JoinCall) -- in the room the two share.  usable: the family takes this plan, set and capacity; passes_bytes: what its
 * join reports for `capacity` records. */
template <typename Join>
int
scan_then_join (const ScanJoinCall &C, bool usable, size_t passes_bytes, Join join) {
  if (!usable || !C.d_count || !C.d_found || C.capacity >= (1ull << 31) || C.out_capacity >= (1ull << 31) || (C.n_symbols && !C.d_text) ||
      (C.out_capacity && !C.d_out) || (C.capacity && !C.d_tmp))
    return ACM_GPU_E_ARG;
  Carve carve (C.capacity ? C.d_tmp : nullptr); /* (no room: nothing is bound) */
  const ScanRoom L = scan_room_carve (carve, C.plan, passes_bytes, C.capacity, C.n_symbols);
  if (C.capacity && C.tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  if (C.capacity == 0) { /* no room: *d_found says what the records need, and nothing matches */
    if (const int rc = acm_gpu_count_device (C.plan, C.d_text, C.n_symbols, 0, C.d_found, C.stream))
      return rc;
    return no_record (C.plan, nullptr, C.d_count, static_cast<hipStream_t> (C.stream));
  }
  if (const int rc = acm_gpu_scan_ordered_device (C.plan, C.d_text, C.n_symbols, 0, C.pos_base, L.found, C.capacity, C.d_found, L.work, L.work_bytes, C.stream))
    return rc;
  return join (JoinCall{ C.plan, L.found, C.capacity, C.d_found, C.n_symbols, C.pos_base, C.d_offsets, C.n_texts, C.d_out, C.out_capacity, C.d_count, L.work,
                         L.work_bytes, C.stream });
}

/* the arguments every acm_gpu_scan_<join>_host has beside its set; dist: the families with a distance per match, may be NULL */
struct ScanJoinHost {
  ACMPlan *plan;
  const void *text;
  uint64_t n_symbols, pos_base;
  const uint64_t *offsets;
  uint64_t n_texts;
  ACMRecord *out;
  uint32_t *dist;
  uint64_t out_capacity;
  uint64_t *n_found;
};

/* The host form of a fused call.  make (&set) compiles the call's set (which goes away with the call), the text goes up,
 * the record room is the exact number of matches, counted first -- room_ok (set, capacity) or ACM_GPU_E_NOMEM --, then
 * the scratch of tmp_bytes (set, capacity), the output, the offsets, the device call scan (set, ScanJoinCall, d_dist)
 * and the matches (with_dist: and their distances) come down. */
template <typename Set, typename Make, typename RoomOk, typename TmpBytes, typename Scan>
int
scan_join_host (const ScanJoinHost &H, bool with_dist, Make make, RoomOk room_ok, TmpBytes tmp_bytes_of, Scan scan) {
  if (!H.plan || !H.n_found || H.out_capacity >= (1ull << 31) || (H.n_symbols && !H.text) || (H.out_capacity && !H.out) ||
      !optional_offsets_ok (H.offsets, H.n_texts, H.n_symbols) || (H.offsets && H.n_texts == 0 && H.n_symbols))
    return ACM_GPU_E_ARG;
  Set *made = nullptr;
  if (const int rc = make (&made))
    return rc;
  std::unique_ptr<Set, void (*) (Set *)> set (made, set_destroy<Set>);
  HIP_TRY (hipSetDevice (H.plan->device));
  DeviceTemps temps;
  void *d_text = nullptr, *d_tmp = nullptr;
  uint64_t *d_res = nullptr, *d_off = nullptr; /* d_res: the matches, the scan's records */
  ACMRecord *d_out = nullptr;
  uint32_t *d_dist = nullptr;
  uint64_t capacity = 0;
  HOST_TRY (upload_text (temps, H.plan, H.text, H.n_symbols, &d_text));
  HOST_TRY (temps.get (&d_res, 16));
  if (const int rc = count_first (H.plan, d_text, H.n_symbols, d_res, &capacity)) /* the record room: the exact number of matches */
    return rc;
  if (!room_ok (set.get (), capacity))
    return ACM_GPU_E_NOMEM;
  const size_t tmp_bytes = tmp_bytes_of (set.get (), capacity);
  HOST_TRY (temps.get (&d_tmp, tmp_bytes));
  HOST_TRY (temps.get (&d_out, H.out_capacity * 16));
  if (with_dist)
    HOST_TRY (temps.get (&d_dist, H.out_capacity * 4));
  if (H.offsets)
    HOST_TRY (upload_offsets (temps, H.offsets, H.n_texts, &d_off));
  int rc = settle (H.plan,
                   scan (set.get (),
                         ScanJoinCall{ H.plan, d_text, H.n_symbols, H.pos_base, d_off, H.n_texts, capacity, d_out, H.out_capacity, d_res, d_res + 1, d_tmp,
                                       tmp_bytes, nullptr },
                         d_dist),
                   true);
  uint64_t found = 0;
  if (!rc) {
    HOST_TRY (hipMemcpy (&found, d_res + 1, 8, hipMemcpyDeviceToHost));
    if (found > capacity) /* (the room is what the count pass found: never expected) */
      rc = ACM_GPU_E_INTERNAL;
  }
  rc = download_records (rc, d_res, d_out, H.out, H.out_capacity, H.n_found);
  if (!rc && with_dist && H.dist && *H.n_found)
    HOST_TRY (hipMemcpy (H.dist, d_dist, *H.n_found * 4, hipMemcpyDeviceToHost));
  return rc;
}
} // namespace

/* ------------------------------------------------------------------ keyword patterns with don't-care gaps (include/acm_gpu.h, dev_patterns.h)
 * A pattern set compiled into an index inverted by anchor keyword, and the passes that join a record
 * set in canonical order under it: the check of offsets[], the count pass, the prefix over the
 * records' counts, the fill pass, the order pass. */
struct ACMPatterns : DeviceSet {
  uint64_t n_patterns = 0, n_terms = 0, anchor_keywords = 0, longest = 0, max_anchor_postings = 0;
  uint32_t *d_anchor_ptr = nullptr, *d_other_ptr = nullptr;
  uint4 *d_post = nullptr;
  PatternOther *d_other = nullptr;
};

namespace {
JoinRoom
patterns_carve (Carve &c, uint64_t capacity, PatternsK &K) {
  /* ACM_GPU_PATTERNS_TILE=<records>: the passes' tile, a multiple of 64 (tests) */
  join_carve_ctl (c, capacity, tunable ("ACM_GPU_PATTERNS_TILE", PATTERNS_TILE_DEFAULT, PATTERNS_TILE_MIN, PATTERNS_TILE_MAX, Tune::MultWave), K);
  return join_carve_counts (c, capacity, K);
}
} // namespace

extern "C" int
acm_gpu_patterns_create (ACMPlan *plan, const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, ACMPatterns **out) {
  if (!plan || !out)
    return ACM_GPU_E_ARG;
  const uint64_t nk = plan->covered_keywords;
  if (acm_patterns_check (terms, pat_ptr, n_patterns, nk))
    return ACM_GPU_E_ARG;
  const uint64_t n_terms = pat_ptr[n_patterns];
  /* the index: every pattern under its anchor, the term with the greatest offset + length (the lowest
   * index among equals); a keyword's postings by L descending, then pattern id ascending */
  struct Post {
    uint32_t keyword_id, pattern, L, alen;
  };
  std::vector<Post> post (n_patterns);
  std::vector<uint32_t> anchor_ptr (nk + 1, 0), other_ptr (n_patterns + 1, 0);
  std::vector<PatternOther> other (n_terms - n_patterns ? n_terms - n_patterns : 1);
  uint64_t longest = 0;
  for (uint64_t p = 0; p < n_patterns; p++) {
    uint64_t anchor = pat_ptr[p];
    for (uint64_t i = pat_ptr[p] + 1; i < pat_ptr[p + 1]; i++)
      if (terms[i].offset + terms[i].length > terms[anchor].offset + terms[anchor].length)
        anchor = i;
    const uint32_t L = terms[anchor].offset + terms[anchor].length;
    post[p] = Post{ terms[anchor].keyword_id, (uint32_t)p, L, terms[anchor].length };
    longest = std::max<uint64_t> (longest, L);
    uint32_t at = other_ptr[p];
    for (uint64_t i = pat_ptr[p]; i < pat_ptr[p + 1]; i++)
      if (i != anchor)
        other[at++] = PatternOther{ L - (terms[i].offset + terms[i].length), terms[i].length, terms[i].keyword_id };
    other_ptr[p + 1] = at;
  }
  std::sort (post.begin (), post.end (), [] (const Post &a, const Post &b) {
    return a.keyword_id != b.keyword_id ? a.keyword_id < b.keyword_id : a.L != b.L ? a.L > b.L : a.pattern < b.pattern;
  });
  std::vector<uint4> post_dev (n_patterns ? n_patterns : 1);
  for (uint64_t q = 0; q < n_patterns; q++) {
    post_dev[q] = make_uint4 (post[q].pattern, post[q].L, post[q].alen, 0);
    anchor_ptr[post[q].keyword_id + 1]++;
  }
  uint64_t anchor_keywords = 0, max_postings = 0;
  for (uint64_t k = 0; k < nk; k++) {
    anchor_keywords += anchor_ptr[k + 1] != 0;
    max_postings = std::max<uint64_t> (max_postings, anchor_ptr[k + 1]);
    anchor_ptr[k + 1] += anchor_ptr[k];
  }
  HIP_TRY (hipSetDevice (plan->device));
  ACMPatterns *P = new (std::nothrow) ACMPatterns ();
  if (!P)
    return ACM_GPU_E_NOMEM;
  P->device = plan->device;
  P->n_patterns = n_patterns;
  P->n_terms = n_terms;
  P->anchor_keywords = anchor_keywords;
  P->longest = longest;
  P->max_anchor_postings = max_postings;
  P->n_keywords = (uint32_t)nk;
  BlobBuilder b;
  const size_t anchor_ptr_at = b.add (anchor_ptr.data (), anchor_ptr.size () * 4), post_at = b.add (post_dev.data (), post_dev.size () * sizeof (uint4)),
               other_ptr_at = b.add (other_ptr.data (), other_ptr.size () * 4), other_at = b.add (other.data (), other.size () * sizeof (PatternOther));
  if (const int rc = set_upload (P, b))
    return rc;
  P->d_anchor_ptr = b.at<uint32_t> (anchor_ptr_at);
  P->d_post = b.at<uint4> (post_at);
  P->d_other_ptr = b.at<uint32_t> (other_ptr_at);
  P->d_other = b.at<PatternOther> (other_at);
  *out = P;
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_patterns_destroy (ACMPatterns *patterns) {
  set_destroy (patterns);
}

extern "C" int
acm_gpu_patterns_info (const ACMPatterns *patterns, ACMPatternsInfo *info) {
  if (!patterns || !info)
    return ACM_GPU_E_ARG;
  *info = ACMPatternsInfo{ patterns->n_patterns, patterns->n_terms, patterns->anchor_keywords, patterns->longest, patterns->max_anchor_postings };
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_patterns_tmp_bytes (const ACMPlan *plan, const ACMPatterns *patterns, uint64_t n_or_capacity, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: the text of a match is a bisection of offsets[]) */
  if (!plan || !patterns || n_or_capacity >= (1ull << 31))
    return 0;
  Carve c;
  PatternsK K{};
  patterns_carve (c, n_or_capacity, K);
  return c.total ();
}

namespace {
/* acm_gpu_patterns_records_device */
int
patterns_join (const JoinCall &C, const ACMPatterns *patterns) {
  if (!join_args_ok (C, patterns))
    return ACM_GPU_E_ARG;
  ACMPlan *plan = C.plan;
  const uint64_t n = C.n, n_texts = C.n_texts, out_capacity = C.out_capacity;
  hipStream_t st = static_cast<hipStream_t> (C.stream);
  if (n == 0) /* (no record: no match, whatever *d_n says) */
    return no_record (plan, nullptr, C.d_count, st);
  Carve carve (C.d_tmp);
  PatternsK K{};
  const JoinRoom L = patterns_carve (carve, n, K);
  if (C.tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.anchor_ptr = patterns->d_anchor_ptr;
  K.post = patterns->d_post;
  K.other_ptr = patterns->d_other_ptr;
  K.other = patterns->d_other;
  K.n_keywords = patterns->n_keywords;
  bind_join (K, C);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (JoinCtl), st));
  /* 1. */
  if (K.offsets) /* one size, whatever the number of texts */
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + PATTERNS_THREADS - 1) / PATTERNS_THREADS), dim3 (PATTERNS_THREADS), 0, st, K.offsets,
                     K.n_texts, K.n_symbols, &K.ctl->bad, K.error));
  /* 2. */
  HIP_TRY (launch (patterns_count_kernel, capped_grid (plan, K.n_tiles), dim3 (PATTERNS_THREADS), 0, st, K));
  /* 3. */
  HIP_TRY (exclusive_sum (L.cub, L.count, L.first, n + 1, st));
  /* 4. */
  HIP_TRY (launch (patterns_fill_kernel, capped_grid (plan, K.n_tiles), dim3 (PATTERNS_THREADS), 0, st, K));
  /* 5. */
  if (out_capacity > 1)
    HIP_TRY (launch (patterns_order_kernel, capped_grid (plan, (out_capacity + PATTERNS_THREADS - 1) / PATTERNS_THREADS), dim3 (PATTERNS_THREADS), 0, st,
                     static_cast<const JoinK &> (K)));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_patterns_records_device (ACMPlan *plan, const ACMPatterns *patterns, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n,
                                 uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts, ACMRecord *d_out,
                                 uint64_t out_capacity, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  return patterns_join (JoinCall{ plan, d_records, n, d_n, n_symbols, pos_base, d_offsets, n_texts, d_out, out_capacity, d_count, d_tmp, tmp_bytes, stream }, patterns);
}

extern "C" size_t
acm_gpu_scan_patterns_tmp_bytes (const ACMPlan *plan, const ACMPatterns *patterns, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || !patterns || capacity >= (1ull << 31))
    return 0;
  Carve c;
  scan_room_carve (c, plan, acm_gpu_patterns_tmp_bytes (plan, patterns, capacity, n_texts), capacity, n_symbols);
  return c.total ();
}

extern "C" int
acm_gpu_scan_patterns_device (ACMPlan *plan, const ACMPatterns *patterns, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                              const uint64_t *d_offsets, uint64_t n_texts, uint64_t capacity, ACMRecord *d_out, uint64_t out_capacity, uint64_t *d_count,
                              uint64_t *d_found, void *d_tmp, size_t tmp_bytes, void *stream) {
  const ScanJoinCall C{ plan, d_text, n_symbols, pos_base, d_offsets, n_texts, capacity, d_out, out_capacity, d_count, d_found, d_tmp, tmp_bytes, stream };
  return scan_then_join (C, plan && patterns && patterns->device == plan->device, acm_gpu_patterns_tmp_bytes (plan, patterns, capacity, n_texts),
                         [&] (const JoinCall &J) { return patterns_join (J, patterns); });
}

extern "C" int
acm_gpu_scan_patterns_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                            const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, ACMRecord *out, uint64_t out_capacity,
                            uint64_t *n_found) {
  const ScanJoinHost H{ plan, text, n_symbols, pos_base, offsets, n_texts, out, nullptr, out_capacity, n_found };
  return scan_join_host<ACMPatterns> (
    H, false, [&] (ACMPatterns **made) { return acm_gpu_patterns_create (plan, terms, pat_ptr, n_patterns, made); },
    [] (const ACMPatterns *, uint64_t) { return true; },
    [&] (const ACMPatterns *set, uint64_t capacity) { return acm_gpu_scan_patterns_tmp_bytes (plan, set, capacity, n_symbols, n_texts); },
    [] (const ACMPatterns *set, const ScanJoinCall &C, uint32_t *) {
      return acm_gpu_scan_patterns_device (C.plan, set, C.d_text, C.n_symbols, C.pos_base, C.d_offsets, C.n_texts, C.capacity, C.d_out, C.out_capacity, C.d_count,
                                           C.d_found, C.d_tmp, C.tmp_bytes, C.stream);
    });
}

/* ------------------------------------------------------------------ keyword chains with bounded gaps (include/acm_gpu.h, dev_chains.h)
 * A chain set compiled into an index inverted by keyword, and the passes that join a record set in
 * canonical order under it: the check of offsets[], one level pass per term level of the set, the
 * count pass, the prefix over the records' counts, the fill pass, the patterns' order pass. */
struct ACMChains : DeviceSet {
  uint64_t n_chains = 0, n_terms = 0, max_terms = 0, max_gap = 0, max_postings = 0, max_last_postings = 0;
  uint32_t *d_post_ptr = nullptr;
  ChainPost *d_post = nullptr;
};

namespace {
constexpr uint64_t CHAINS_MOST_SLOTS = 1ull << 40; /* state slots of one call: records x the most postings of a keyword */

JoinRoom
chains_carve (Carve &c, const ACMChains *chains, uint64_t capacity, ChainsK &K) {
  /* ACM_GPU_CHAINS_TILE=<records>: the passes' tile, a multiple of 64 (tests); ACM_GPU_CHAINS_COOP=<records>: windows of more
   * records are walked by the whole wave (0: every window, a huge value: none) */
  join_carve_ctl (c, capacity, tunable ("ACM_GPU_CHAINS_TILE", CHAINS_TILE_DEFAULT, CHAINS_TILE_MIN, CHAINS_TILE_MAX, Tune::MultWave), K);
  K.coop = tunable ("ACM_GPU_CHAINS_COOP", CHAINS_COOP_DEFAULT, 0, 0x7FFFFFFFu, Tune::Any);
  K.stride = (uint32_t)std::max<uint64_t> (chains->max_postings, 1);
  K.state = c.take<unsigned long long> ((size_t)(capacity * K.stride));
  return join_carve_counts (c, capacity, K);
}

bool
chains_room_ok (const ACMChains *chains, uint64_t capacity) {
  return capacity < (1ull << 31) && capacity * std::max<uint64_t> (chains->max_postings, 1) < CHAINS_MOST_SLOTS;
}
} // namespace

extern "C" int
acm_gpu_chains_create (ACMPlan *plan, const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, ACMChains **out) {
  if (!plan || !out)
    return ACM_GPU_E_ARG;
  const uint64_t nk = plan->covered_keywords;
  if (acm_chains_check (terms, chain_ptr, n_chains, nk))
    return ACM_GPU_E_ARG;
  const uint64_t n_terms = chain_ptr[n_chains];
  /* the index: every term under its keyword, a keyword's postings by level, then chain */
  struct Place {
    uint32_t keyword_id, level, chain, term;
  };
  std::vector<Place> place (n_terms);
  std::vector<uint32_t> post_ptr (nk + 1, 0), last_of (nk + 1, 0), at_of (n_terms ? n_terms : 1);
  uint64_t max_terms = 0, max_gap = 0;
  for (uint64_t c = 0; c < n_chains; c++) {
    max_terms = std::max (max_terms, chain_ptr[c + 1] - chain_ptr[c]);
    for (uint64_t i = chain_ptr[c]; i < chain_ptr[c + 1]; i++) {
      place[i] = Place{ terms[i].keyword_id, (uint32_t)(i - chain_ptr[c]), (uint32_t)c, (uint32_t)i };
      max_gap = std::max<uint64_t> (max_gap, terms[i].gap_max);
      post_ptr[terms[i].keyword_id + 1]++;
      last_of[terms[i].keyword_id] += i + 1 == chain_ptr[c + 1];
    }
  }
  std::sort (place.begin (), place.end (), [] (const Place &a, const Place &b) {
    return a.keyword_id != b.keyword_id ? a.keyword_id < b.keyword_id : a.level != b.level ? a.level < b.level : a.chain < b.chain;
  });
  uint64_t max_postings = 0, max_last = 0;
  for (uint64_t k = 0; k < nk; k++) {
    max_postings = std::max<uint64_t> (max_postings, post_ptr[k + 1]);
    max_last = std::max<uint64_t> (max_last, last_of[k]);
    post_ptr[k + 1] += post_ptr[k];
  }
  for (uint64_t q = 0; q < n_terms; q++) /* where a term stands among its keyword's postings */
    at_of[place[q].term] = (uint32_t)(q - post_ptr[place[q].keyword_id]);
  std::vector<ChainPost> post (n_terms ? n_terms : 1);
  for (uint64_t q = 0; q < n_terms; q++) {
    const Place &p = place[q];
    const ACMChainTerm &t = terms[p.term];
    const bool last = p.term + 1 == chain_ptr[p.chain + 1];
    post[q] = ChainPost{ p.chain, p.level | (last ? CHAINS_LAST : 0), t.gap_min, t.gap_max, p.level ? terms[p.term - 1].keyword_id : 0,
                         p.level ? at_of[p.term - 1] : 0, { 0, 0 } };
  }
  HIP_TRY (hipSetDevice (plan->device));
  ACMChains *S = new (std::nothrow) ACMChains ();
  if (!S)
    return ACM_GPU_E_NOMEM;
  S->device = plan->device;
  S->n_chains = n_chains;
  S->n_terms = n_terms;
  S->max_terms = max_terms;
  S->max_gap = max_gap;
  S->max_postings = max_postings;
  S->max_last_postings = max_last;
  S->n_keywords = (uint32_t)nk;
  BlobBuilder b;
  const size_t post_ptr_at = b.add (post_ptr.data (), post_ptr.size () * 4), post_at = b.add (post.data (), post.size () * sizeof (ChainPost));
  if (const int rc = set_upload (S, b))
    return rc;
  S->d_post_ptr = b.at<uint32_t> (post_ptr_at);
  S->d_post = b.at<ChainPost> (post_at);
  *out = S;
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_chains_destroy (ACMChains *chains) {
  set_destroy (chains);
}

extern "C" int
acm_gpu_chains_info (const ACMChains *chains, ACMChainsInfo *info) {
  if (!chains || !info)
    return ACM_GPU_E_ARG;
  *info = ACMChainsInfo{ chains->n_chains, chains->n_terms, chains->max_terms, chains->max_gap, chains->max_postings, chains->max_last_postings };
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_chains_tmp_bytes (const ACMPlan *plan, const ACMChains *chains, uint64_t n_or_capacity, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: the text of a match is a bisection of offsets[]) */
  if (!plan || !chains || !chains_room_ok (chains, n_or_capacity))
    return 0;
  Carve c;
  ChainsK K{};
  chains_carve (c, chains, n_or_capacity, K);
  return c.total ();
}

namespace {
/* acm_gpu_chains_records_device */
int
chains_join (const JoinCall &C, const ACMChains *chains) {
  if (!join_args_ok (C, chains) || !chains_room_ok (chains, C.n))
    return ACM_GPU_E_ARG;
  ACMPlan *plan = C.plan;
  const uint64_t n = C.n, n_texts = C.n_texts, out_capacity = C.out_capacity;
  hipStream_t st = static_cast<hipStream_t> (C.stream);
  if (n == 0) /* (no record: no match, whatever *d_n says) */
    return no_record (plan, nullptr, C.d_count, st);
  Carve carve (C.d_tmp);
  ChainsK K{};
  const JoinRoom L = chains_carve (carve, chains, n, K);
  if (C.tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.post_ptr = chains->d_post_ptr;
  K.post = chains->d_post;
  K.n_keywords = chains->n_keywords;
  bind_join (K, C);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (JoinCtl), st));
  /* the check */
  if (K.offsets) /* one size, whatever the number of texts */
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + PATTERNS_THREADS - 1) / PATTERNS_THREADS), dim3 (PATTERNS_THREADS), 0, st, K.offsets,
                     K.n_texts, K.n_symbols, &K.ctl->bad, K.error));
  /* 1. (as many launches as the set's longest chain has terms) */
  for (uint32_t level = 0; level < chains->max_terms; level++) {
    K.level = level;
    HIP_TRY (launch (chains_level_kernel, capped_grid (plan, K.n_tiles), dim3 (CHAINS_THREADS), 0, st, K));
  }
  /* 2. */
  HIP_TRY (launch (chains_count_kernel, capped_grid (plan, K.n_tiles), dim3 (CHAINS_THREADS), 0, st, K));
  /* 3. */
  HIP_TRY (exclusive_sum (L.cub, L.count, L.first, n + 1, st));
  /* 4. */
  HIP_TRY (launch (chains_fill_kernel, capped_grid (plan, K.n_tiles), dim3 (CHAINS_THREADS), 0, st, K));
  /* 5. (dev_patterns.h's, which reads the head of K alone) */
  if (out_capacity > 1)
    HIP_TRY (launch (patterns_order_kernel, capped_grid (plan, (out_capacity + PATTERNS_THREADS - 1) / PATTERNS_THREADS), dim3 (PATTERNS_THREADS), 0, st,
                     static_cast<const JoinK &> (K)));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_chains_records_device (ACMPlan *plan, const ACMChains *chains, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, uint64_t n_symbols,
                               uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts, ACMRecord *d_out, uint64_t out_capacity,
                               uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  return chains_join (JoinCall{ plan, d_records, n, d_n, n_symbols, pos_base, d_offsets, n_texts, d_out, out_capacity, d_count, d_tmp, tmp_bytes, stream }, chains);
}

extern "C" size_t
acm_gpu_scan_chains_tmp_bytes (const ACMPlan *plan, const ACMChains *chains, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || !chains || !chains_room_ok (chains, capacity))
    return 0;
  Carve c;
  scan_room_carve (c, plan, acm_gpu_chains_tmp_bytes (plan, chains, capacity, n_texts), capacity, n_symbols);
  return c.total ();
}

extern "C" int
acm_gpu_scan_chains_device (ACMPlan *plan, const ACMChains *chains, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets,
                            uint64_t n_texts, uint64_t capacity, ACMRecord *d_out, uint64_t out_capacity, uint64_t *d_count, uint64_t *d_found,
                            void *d_tmp, size_t tmp_bytes, void *stream) {
  const ScanJoinCall C{ plan, d_text, n_symbols, pos_base, d_offsets, n_texts, capacity, d_out, out_capacity, d_count, d_found, d_tmp, tmp_bytes, stream };
  return scan_then_join (C, plan && chains && chains->device == plan->device && chains_room_ok (chains, capacity),
                         acm_gpu_chains_tmp_bytes (plan, chains, capacity, n_texts), [&] (const JoinCall &J) { return chains_join (J, chains); });
}

extern "C" int
acm_gpu_scan_chains_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                          const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, ACMRecord *out, uint64_t out_capacity,
                          uint64_t *n_found) {
  const ScanJoinHost H{ plan, text, n_symbols, pos_base, offsets, n_texts, out, nullptr, out_capacity, n_found };
  return scan_join_host<ACMChains> (
    H, false, [&] (ACMChains **made) { return acm_gpu_chains_create (plan, terms, chain_ptr, n_chains, made); }, chains_room_ok,
    [&] (const ACMChains *set, uint64_t capacity) { return acm_gpu_scan_chains_tmp_bytes (plan, set, capacity, n_symbols, n_texts); },
    [] (const ACMChains *set, const ScanJoinCall &C, uint32_t *) {
      return acm_gpu_scan_chains_device (C.plan, set, C.d_text, C.n_symbols, C.pos_base, C.d_offsets, C.n_texts, C.capacity, C.d_out, C.out_capacity, C.d_count,
                                         C.d_found, C.d_tmp, C.tmp_bytes, C.stream);
    });
}

/* ------------------------------------------------------------------ unordered keyword proximity (include/acm_near.h, dev_near.h)
 * A group set compiled into an index inverted by keyword, and the passes that join a record set in
 * canonical order under it: the check of offsets[], the walk pass, the count pass, the prefix over
 * the records' counts, the fill pass, the patterns' order pass. */
struct ACMNear : DeviceSet {
  uint64_t n_groups = 0, n_terms = 0, max_terms = 0, max_width = 0, max_postings = 0;
  uint32_t *d_post_ptr = nullptr;
  NearPost *d_post = nullptr;
};

namespace {
constexpr uint64_t NEAR_MOST_SLOTS = 1ull << 40; /* slots of one call: records x the most postings of a keyword */

JoinRoom
near_carve (Carve &c, const ACMNear *near, uint64_t capacity, NearK &K) {
  /* ACM_GPU_NEAR_TILE=<records>: the passes' tile, a multiple of 64 (tests); ACM_GPU_NEAR_COOP=<records>: walks of more records are
   * finished by the whole wave (0: every walk, a huge value: none).  COOP's default is CHAINS' own; the tile's is the best of the four
   * that tools/exp_near.py measured (dev_near.h). */
  join_carve_ctl (c, capacity, tunable ("ACM_GPU_NEAR_TILE", NEAR_TILE_DEFAULT, NEAR_TILE_MIN, NEAR_TILE_MAX, Tune::MultWave), K);
  K.coop = tunable ("ACM_GPU_NEAR_COOP", NEAR_COOP_DEFAULT, 0, 0x7FFFFFFFu, Tune::Any);
  K.stride = (uint32_t)std::max<uint64_t> (near->max_postings, 1);
  K.state = c.take<unsigned long long> ((size_t)(capacity * K.stride));
  return join_carve_counts (c, capacity, K);
}

bool
near_room_ok (const ACMNear *near, uint64_t capacity) {
  return capacity < (1ull << 31) && capacity * std::max<uint64_t> (near->max_postings, 1) < NEAR_MOST_SLOTS;
}
} // namespace

extern "C" int
acm_gpu_near_create (ACMPlan *plan, const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups, ACMNear **out) {
  if (!plan || !out)
    return ACM_GPU_E_ARG;
  const uint64_t nk = plan->covered_keywords;
  if (acm_near_check (terms, group_ptr, groups, n_groups, nk))
    return ACM_GPU_E_ARG;
  const uint64_t n_terms = group_ptr[n_groups];
  /* the index: every term under its keyword, a keyword's postings by group (a counting sort over the groups in order) */
  std::vector<uint32_t> post_ptr (nk + 1, 0), at (nk, 0);
  uint64_t max_terms = 0, max_width = 0, max_postings = 0;
  for (uint64_t i = 0; i < n_terms; i++)
    post_ptr[terms[i] + 1]++;
  for (uint64_t k = 0; k < nk; k++) {
    max_postings = std::max<uint64_t> (max_postings, post_ptr[k + 1]);
    post_ptr[k + 1] += post_ptr[k];
    at[k] = post_ptr[k];
  }
  std::vector<NearPost> post (n_terms ? n_terms : 1);
  for (uint64_t g = 0; g < n_groups; g++) {
    const uint64_t m = group_ptr[g + 1] - group_ptr[g], need = groups[g].need ? groups[g].need : m;
    max_terms = std::max (max_terms, m);
    max_width = std::max<uint64_t> (max_width, groups[g].width);
    for (uint64_t j = 0; j < m; j++)
      post[at[terms[group_ptr[g] + j]]++] = NearPost{ (uint32_t)g, groups[g].width, (uint32_t)(j | m << 8 | need << 16), 0 };
  }
  HIP_TRY (hipSetDevice (plan->device));
  ACMNear *S = new (std::nothrow) ACMNear ();
  if (!S)
    return ACM_GPU_E_NOMEM;
  S->device = plan->device;
  S->n_groups = n_groups;
  S->n_terms = n_terms;
  S->max_terms = max_terms;
  S->max_width = max_width;
  S->max_postings = max_postings;
  S->n_keywords = (uint32_t)nk;
  BlobBuilder b;
  const size_t post_ptr_at = b.add (post_ptr.data (), post_ptr.size () * 4), post_at = b.add (post.data (), post.size () * sizeof (NearPost));
  if (const int rc = set_upload (S, b))
    return rc;
  S->d_post_ptr = b.at<uint32_t> (post_ptr_at);
  S->d_post = b.at<NearPost> (post_at);
  *out = S;
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_near_destroy (ACMNear *near) {
  set_destroy (near);
}

extern "C" int
acm_gpu_near_info (const ACMNear *near, ACMNearInfo *info) {
  if (!near || !info)
    return ACM_GPU_E_ARG;
  *info = ACMNearInfo{ near->n_groups, near->n_terms, near->max_terms, near->max_width, near->max_postings };
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_near_tmp_bytes (const ACMPlan *plan, const ACMNear *near, uint64_t n_or_capacity, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: the text of an end is a bisection of offsets[]) */
  if (!plan || !near || !near_room_ok (near, n_or_capacity))
    return 0;
  Carve c;
  NearK K{};
  near_carve (c, near, n_or_capacity, K);
  return c.total ();
}

namespace {
/* acm_gpu_near_records_device */
int
near_join (const JoinCall &C, const ACMNear *near) {
  if (!join_args_ok (C, near) || !near_room_ok (near, C.n))
    return ACM_GPU_E_ARG;
  ACMPlan *plan = C.plan;
  const uint64_t n = C.n, n_texts = C.n_texts, out_capacity = C.out_capacity;
  hipStream_t st = static_cast<hipStream_t> (C.stream);
  if (n == 0) /* (no record: no match, whatever *d_n says) */
    return no_record (plan, nullptr, C.d_count, st);
  Carve carve (C.d_tmp);
  NearK K{};
  const JoinRoom L = near_carve (carve, near, n, K);
  if (C.tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  K.post_ptr = near->d_post_ptr;
  K.post = near->d_post;
  K.n_keywords = near->n_keywords;
  bind_join (K, C);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (JoinCtl), st));
  /* the check */
  if (K.offsets) /* one size, whatever the number of texts */
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + PATTERNS_THREADS - 1) / PATTERNS_THREADS), dim3 (PATTERNS_THREADS), 0, st, K.offsets,
                     K.n_texts, K.n_symbols, &K.ctl->bad, K.error));
  /* 1. (one launch, whatever the groups hold) */
  HIP_TRY (launch (near_walk_kernel, capped_grid (plan, K.n_tiles), dim3 (NEAR_THREADS), 0, st, K));
  /* 2. */
  HIP_TRY (launch (near_count_kernel, capped_grid (plan, K.n_tiles), dim3 (NEAR_THREADS), 0, st, K));
  /* 3. */
  HIP_TRY (exclusive_sum (L.cub, L.count, L.first, n + 1, st));
  /* 4. */
  HIP_TRY (launch (near_fill_kernel, capped_grid (plan, K.n_tiles), dim3 (NEAR_THREADS), 0, st, K));
  /* 5. (dev_patterns.h's, which reads the head of K alone) */
  if (out_capacity > 1)
    HIP_TRY (launch (patterns_order_kernel, capped_grid (plan, (out_capacity + PATTERNS_THREADS - 1) / PATTERNS_THREADS), dim3 (PATTERNS_THREADS), 0, st,
                     static_cast<const JoinK &> (K)));
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_near_records_device (ACMPlan *plan, const ACMNear *near, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, uint64_t n_symbols,
                             uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts, ACMRecord *d_out, uint64_t out_capacity, uint64_t *d_count,
                             void *d_tmp, size_t tmp_bytes, void *stream) {
  return near_join (JoinCall{ plan, d_records, n, d_n, n_symbols, pos_base, d_offsets, n_texts, d_out, out_capacity, d_count, d_tmp, tmp_bytes, stream }, near);
}

extern "C" size_t
acm_gpu_scan_near_tmp_bytes (const ACMPlan *plan, const ACMNear *near, uint64_t capacity, uint64_t n_symbols, uint64_t n_texts) {
  if (!plan || !near || !near_room_ok (near, capacity))
    return 0;
  Carve c;
  scan_room_carve (c, plan, acm_gpu_near_tmp_bytes (plan, near, capacity, n_texts), capacity, n_symbols);
  return c.total ();
}

extern "C" int
acm_gpu_scan_near_device (ACMPlan *plan, const ACMNear *near, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets,
                          uint64_t n_texts, uint64_t capacity, ACMRecord *d_out, uint64_t out_capacity, uint64_t *d_count, uint64_t *d_found, void *d_tmp,
                          size_t tmp_bytes, void *stream) {
  const ScanJoinCall C{ plan, d_text, n_symbols, pos_base, d_offsets, n_texts, capacity, d_out, out_capacity, d_count, d_found, d_tmp, tmp_bytes, stream };
  return scan_then_join (C, plan && near && near->device == plan->device && near_room_ok (near, capacity),
                         acm_gpu_near_tmp_bytes (plan, near, capacity, n_texts), [&] (const JoinCall &J) { return near_join (J, near); });
}

extern "C" int
acm_gpu_scan_near_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                        const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups, ACMRecord *out,
                        uint64_t out_capacity, uint64_t *n_found) {
  const ScanJoinHost H{ plan, text, n_symbols, pos_base, offsets, n_texts, out, nullptr, out_capacity, n_found };
  return scan_join_host<ACMNear> (
    H, false, [&] (ACMNear **made) { return acm_gpu_near_create (plan, terms, group_ptr, groups, n_groups, made); }, near_room_ok,
    [&] (const ACMNear *set, uint64_t capacity) { return acm_gpu_scan_near_tmp_bytes (plan, set, capacity, n_symbols, n_texts); },
    [] (const ACMNear *set, const ScanJoinCall &C, uint32_t *) {
      return acm_gpu_scan_near_device (C.plan, set, C.d_text, C.n_symbols, C.pos_base, C.d_offsets, C.n_texts, C.capacity, C.d_out, C.out_capacity, C.d_count,
                                       C.d_found, C.d_tmp, C.tmp_bytes, C.stream);
    });
}

/* ------------------------------------------------------------------ keywords with up to k mismatches (include/acm_gpu.h, dev_approx.h)
 * A target set compiled into an index inverted by term keyword, and the passes that verify a record set in
 * canonical order under it: the check of offsets[], the count pass, the prefix over the records' counts, the
 * fill pass, the two sorts of the order and the gather. */
struct ACMApprox : DeviceSet {
  uint64_t n_targets = 0, n_terms = 0, seed_keywords = 0, longest = 0, max_k = 0, max_postings = 0;
  uint32_t sym_bytes = 0;
  bool edit_fit = false; /* every k[w] <= 15 and < L_w: the edit calls take the set (acm_edit_check's two conditions) */
  uint32_t *d_post_ptr = nullptr;
  uint4 *d_post = nullptr, *d_target = nullptr;
  uint64_t *d_spell_off = nullptr;
  ApproxTerm *d_terms = nullptr;
  void *d_spell = nullptr;
  /* a template set (dev_templates.h): the cells and the compiled classes; d_cells stays NULL in a target set */
  uint64_t n_classes = 0;
  uint32_t *d_cells = nullptr, *d_cls_bitmap = nullptr, *d_cls_flags = nullptr;
  uint64_t *d_cls_ptr = nullptr;
  void *d_cls_ranges = nullptr;
};

/* a template set is a target set whose positions are cells */
struct ACMTemplates {
  ACMApprox *set = nullptr;
};

namespace {
/* bits that hold every value in [0, most] */
uint32_t
bits_of (uint64_t most) {
  uint32_t bits = 1;
  while (bits < 64 && (most >> bits))
    bits++;
  return bits;
}

size_t
approx_sort_bytes (uint64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs (nullptr, bytes, static_cast<const uint64_t *> (nullptr), static_cast<uint64_t *> (nullptr),
                                            static_cast<const uint32_t *> (nullptr), static_cast<uint32_t *> (nullptr), (int)n, 0, 64, nullptr);
  return bytes;
}

/* what approx_carve derives beside K's pointers: the join's counts and sums, the order's two key and index buffers */
struct ApproxRoom : JoinRoom {
  uint64_t *key_a = nullptr, *key_b = nullptr;
  uint32_t *idx_a = nullptr, *idx_b = nullptr;
  void *sort = nullptr;
  size_t sort_bytes = 0;
};
ApproxRoom
approx_carve (Carve &c, uint64_t capacity, uint64_t out_capacity, ApproxK &K) {
  ApproxRoom R;
  /* ACM_GPU_APPROX_TILE=<records>: the passes' tile, a multiple of 64 (tests) */
  join_carve_ctl (c, capacity, tunable ("ACM_GPU_APPROX_TILE", APPROX_TILE_DEFAULT, APPROX_TILE_MIN, APPROX_TILE_MAX, Tune::MultWave), K);
  static_cast<JoinRoom &> (R) = join_carve_counts (c, capacity, K);
  if (out_capacity) {
    K.fill = c.take<ACMRecord> ((size_t)out_capacity);
    K.fill_dist = c.take<uint32_t> ((size_t)out_capacity);
    R.key_a = c.take<uint64_t> ((size_t)out_capacity);
    R.key_b = c.take<uint64_t> ((size_t)out_capacity);
    R.idx_a = c.take<uint32_t> ((size_t)out_capacity);
    R.idx_b = c.take<uint32_t> ((size_t)out_capacity);
    R.sort_bytes = approx_sort_bytes (out_capacity);
    R.sort = c.take (R.sort_bytes + 16);
  }
  return R;
}

template <typename T, bool CELLS>
int
approx_passes (ACMPlan *plan, ApproxK &K, const ApproxRoom &L, uint64_t n, uint64_t n_texts, hipStream_t st) {
  /* 1. */
  if (K.offsets) /* one size, whatever the number of texts */
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + APPROX_THREADS - 1) / APPROX_THREADS), dim3 (APPROX_THREADS), 0, st, K.offsets,
                     K.n_texts, K.n_symbols, &K.ctl->bad, K.error));
  /* 2. */
  HIP_TRY (launch (approx_count_kernel<T, CELLS>, capped_grid (plan, K.n_tiles), dim3 (APPROX_THREADS), 0, st, K));
  /* 3. */
  HIP_TRY (exclusive_sum (L.cub, L.count, L.first, n + 1, st));
  /* 4. */
  HIP_TRY (launch (approx_fill_kernel<T, CELLS>, capped_grid (plan, K.n_tiles), dim3 (APPROX_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

/* ---- keywords within edit distance k (include/acm_gpu.h, dev_edit.h).  The set is ACMApprox and the passes are the ones above; the
 * count and fill kernels are dev_edit.h's, with the group width fixed per call from the set's max_k.  The metric is a property of the
 * call, so the entry points of both metrics are one body each (set_records_device, scan_set_device, scan_set_host). */
enum class Metric { Mismatches, Edits, Templates }; /* Templates: mismatches of cells, over a template set (dev_templates.h) */

/* whether the calls of a metric take this plan and set */
bool
set_usable (Metric metric, const ACMPlan *plan, const ACMApprox *approx) {
  return plan && approx && approx->device == plan->device && approx->sym_bytes == plan->text_sym_bytes && !plan->class_sym_bytes &&
         (metric == Metric::Templates) == (approx->d_cells != nullptr) && (metric != Metric::Edits || approx->edit_fit);
}

/* approx_carve; the edit passes have a tile of their own */
ApproxRoom
set_carve (Metric metric, Carve &c, uint64_t capacity, uint64_t out_capacity, ApproxK &K) {
  const ApproxRoom R = approx_carve (c, capacity, out_capacity, K);
  if (metric == Metric::Edits) {
    /* ACM_GPU_EDIT_TILE=<records>: the passes' tile, a multiple of 64 (tests) */
    K.tile = tunable ("ACM_GPU_EDIT_TILE", EDIT_TILE_DEFAULT, EDIT_TILE_MIN, EDIT_TILE_MAX, Tune::MultWave);
    K.n_tiles = (capacity + K.tile - 1) / K.tile;
  }
  if (metric == Metric::Templates) {
    /* ACM_GPU_TEMPLATES_TILE=<records>: the passes' tile, a multiple of 64 (tests) */
    K.tile = tunable ("ACM_GPU_TEMPLATES_TILE", APPROX_TILE_DEFAULT, APPROX_TILE_MIN, APPROX_TILE_MAX, Tune::MultWave);
    K.n_tiles = (capacity + K.tile - 1) / K.tile;
  }
  return R;
}

size_t
set_tmp_bytes (Metric metric, const ACMPlan *plan, const ACMApprox *approx, uint64_t n_or_capacity, uint64_t out_capacity) {
  if (!set_usable (metric, plan, approx) || n_or_capacity >= (1ull << 31) || out_capacity >= (1ull << 31))
    return 0;
  Carve c;
  ApproxK K{};
  set_carve (metric, c, n_or_capacity, out_capacity, K);
  return c.total ();
}

template <typename T, uint32_t G>
int
edit_passes (ACMPlan *plan, ApproxK &K, const ApproxRoom &L, uint64_t n, uint64_t n_texts, hipStream_t st) {
  if (K.offsets)
    HIP_TRY (launch (offsets_check_kernel, capped_grid (plan, (n_texts + APPROX_THREADS - 1) / APPROX_THREADS), dim3 (APPROX_THREADS), 0, st, K.offsets,
                     K.n_texts, K.n_symbols, &K.ctl->bad, K.error));
  HIP_TRY (launch (edit_count_kernel<T, G>, capped_grid (plan, K.n_tiles), dim3 (EDIT_THREADS), 0, st, K));
  HIP_TRY (exclusive_sum (L.cub, L.count, L.first, n + 1, st));
  HIP_TRY (launch (edit_fill_kernel<T, G>, capped_grid (plan, K.n_tiles), dim3 (EDIT_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

/* the passes of a call: APPROX's, or EDIT's at the group width of the set (a band is at most 4 k + 1 diagonals wide) */
template <typename T>
int
set_passes (Metric metric, uint64_t max_k, ACMPlan *plan, ApproxK &K, const ApproxRoom &L, uint64_t n, uint64_t n_texts, hipStream_t st) {
  if (metric == Metric::Mismatches)
    return approx_passes<T, false> (plan, K, L, n, n_texts, st);
  if (metric == Metric::Templates)
    return approx_passes<T, true> (plan, K, L, n, n_texts, st);
  if (max_k <= 3)
    return edit_passes<T, 16> (plan, K, L, n, n_texts, st);
  if (max_k <= 7)
    return edit_passes<T, 32> (plan, K, L, n, n_texts, st);
  return edit_passes<T, 64> (plan, K, L, n, n_texts, st);
}
} // namespace

namespace {
/* the classes of a template set as the device reads them (dev_templates.h): bitmaps for 1-byte symbols, else pointers, ranges, flags */
struct ClassTables {
  std::vector<uint32_t> bitmap, flags;
  std::vector<uint64_t> ptr;
};
ClassTables
compile_classes (const ACMTemplateSpec *T, uint32_t sb) {
  ClassTables C;
  if (sb == 1) {
    const unsigned char *ranges = static_cast<const unsigned char *> (T->ranges);
    C.bitmap.assign ((size_t)T->n_classes * 8, 0);
    for (uint64_t c = 0; c < T->n_classes; c++) {
      uint32_t *words = &C.bitmap[(size_t)c * 8];
      for (uint64_t r = T->cls_ptr[c]; r < T->cls_ptr[c + 1]; r++)
        for (uint32_t x = ranges[2 * r]; x <= ranges[2 * r + 1]; x++)
          words[x >> 5] |= 1u << (x & 31);
      if (T->cls_flags[c] & ACM_TEMPLATE_NEGATED)
        for (uint32_t i = 0; i < 8; i++)
          words[i] = ~words[i];
    }
  } else {
    C.ptr.assign (1, 0);
    if (T->n_classes) {
      C.ptr.assign (T->cls_ptr, T->cls_ptr + T->n_classes + 1);
      C.flags.assign (T->cls_flags, T->cls_flags + T->n_classes);
    }
  }
  return C;
}

/* acm_gpu_approx_create; with `tpl`, whose arrays the other arguments are, a template set (the caller has run acm_templates_check) */
int
set_create (ACMPlan *plan, const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr,
            uint64_t n_targets, const ACMTemplateSpec *tpl, ACMApprox **out) {
  if (!plan || !out || (n_targets && !spell_data))
    return ACM_GPU_E_ARG;
  const uint64_t nk = plan->covered_keywords;
  if (acm_approx_check (spell_off, k, terms, tgt_ptr, n_targets, nk))
    return ACM_GPU_E_ARG;
  if (plan->class_sym_bytes) /* verification is bitwise on the caller's text */
    return ACM_GPU_E_INELIGIBLE;
  const uint64_t n_terms = tgt_ptr[n_targets], n_spell = spell_off[n_targets];
  const uint32_t sb = plan->text_sym_bytes;
  /* the index: every term under its keyword; a keyword's postings by target id, then term index */
  struct Post {
    uint32_t keyword_id, target, j, offset, length;
  };
  std::vector<Post> post (n_terms);
  std::vector<uint32_t> post_ptr (nk + 1, 0);
  std::vector<uint4> target (n_targets ? n_targets : 1);
  std::vector<uint64_t> first_symbol (n_targets ? n_targets : 1);
  std::vector<ApproxTerm> term_dev (n_terms ? n_terms : 1);
  uint64_t longest = 0, max_k = 0;
  bool edit_fit = true;
  for (uint64_t w = 0; w < n_targets; w++) {
    const uint64_t L = spell_off[w + 1] - spell_off[w];
    edit_fit = edit_fit && k[w] <= EDIT_MAX_K && k[w] < L;
    target[w] = make_uint4 ((uint32_t)L, k[w], (uint32_t)tgt_ptr[w], 0);
    first_symbol[w] = spell_off[w];
    longest = std::max (longest, L);
    max_k = std::max<uint64_t> (max_k, k[w]);
    for (uint64_t i = tgt_ptr[w]; i < tgt_ptr[w + 1]; i++) {
      post[i] = Post{ terms[i].keyword_id, (uint32_t)w, (uint32_t)(i - tgt_ptr[w]), terms[i].offset, terms[i].length };
      term_dev[i] = ApproxTerm{ terms[i].offset, terms[i].length, terms[i].keyword_id };
    }
  }
  std::sort (post.begin (), post.end (), [] (const Post &a, const Post &b) {
    return a.keyword_id != b.keyword_id ? a.keyword_id < b.keyword_id : a.target != b.target ? a.target < b.target : a.j < b.j;
  });
  std::vector<uint4> post_dev (n_terms ? n_terms : 1);
  for (uint64_t q = 0; q < n_terms; q++) {
    post_dev[q] = make_uint4 (post[q].target, post[q].j, post[q].offset, post[q].length);
    post_ptr[post[q].keyword_id + 1]++;
  }
  uint64_t seed_keywords = 0, max_postings = 0;
  for (uint64_t kw = 0; kw < nk; kw++) {
    seed_keywords += post_ptr[kw + 1] != 0;
    max_postings = std::max<uint64_t> (max_postings, post_ptr[kw + 1]);
    post_ptr[kw + 1] += post_ptr[kw];
  }
  HIP_TRY (hipSetDevice (plan->device));
  ACMApprox *A = new (std::nothrow) ACMApprox ();
  if (!A)
    return ACM_GPU_E_NOMEM;
  A->device = plan->device;
  A->n_targets = n_targets;
  A->n_terms = n_terms;
  A->seed_keywords = seed_keywords;
  A->longest = longest;
  A->max_k = max_k;
  A->edit_fit = edit_fit;
  A->max_postings = max_postings;
  A->n_keywords = (uint32_t)nk;
  A->sym_bytes = sb;
  BlobBuilder b;
  const size_t spell_bytes = (size_t)n_spell * sb;
  const size_t post_ptr_at = b.add (post_ptr.data (), post_ptr.size () * 4), post_at = b.add (post_dev.data (), post_dev.size () * sizeof (uint4)),
               target_at = b.add (target.data (), target.size () * sizeof (uint4)), first_at = b.add (first_symbol.data (), first_symbol.size () * 8),
               terms_at = b.add (term_dev.data (), term_dev.size () * sizeof (ApproxTerm)), spell_at = b.add (spell_data, spell_bytes, spell_bytes + 16);
  /* a template set: the cells, and the classes in the form the symbol size reads (every array with room, so that none is NULL) */
  ClassTables classes;
  size_t cells_at = 0, bitmap_at = 0, cls_ptr_at = 0, ranges_at = 0, flags_at = 0;
  if (tpl) {
    classes = compile_classes (tpl, sb);
    const size_t range_bytes = sb == 1 ? 0 : (size_t)classes.ptr.back () * 2 * sb;
    cells_at = b.add (tpl->cells, (size_t)n_spell * 4, (size_t)n_spell * 4 + 16);
    bitmap_at = b.add (classes.bitmap.data (), classes.bitmap.size () * 4, classes.bitmap.size () * 4 + 16);
    cls_ptr_at = b.add (classes.ptr.data (), classes.ptr.size () * 8, classes.ptr.size () * 8 + 16);
    ranges_at = b.add (tpl->ranges, range_bytes, range_bytes + 16);
    flags_at = b.add (classes.flags.data (), classes.flags.size () * 4, classes.flags.size () * 4 + 16);
  }
  if (const int rc = set_upload (A, b))
    return rc;
  if (tpl) {
    A->n_classes = tpl->n_classes;
    A->d_cells = b.at<uint32_t> (cells_at);
    A->d_cls_bitmap = b.at<uint32_t> (bitmap_at);
    A->d_cls_ptr = b.at<uint64_t> (cls_ptr_at);
    A->d_cls_ranges = b.at<> (ranges_at);
    A->d_cls_flags = b.at<uint32_t> (flags_at);
  }
  A->d_post_ptr = b.at<uint32_t> (post_ptr_at);
  A->d_post = b.at<uint4> (post_at);
  A->d_target = b.at<uint4> (target_at);
  A->d_spell_off = b.at<uint64_t> (first_at);
  A->d_terms = b.at<ApproxTerm> (terms_at);
  A->d_spell = b.at<> (spell_at);
  *out = A;
  return ACM_GPU_OK;
}
} // namespace

extern "C" int
acm_gpu_approx_create (ACMPlan *plan, const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms,
                       const uint64_t *tgt_ptr, uint64_t n_targets, ACMApprox **out) {
  return set_create (plan, spell_data, spell_off, k, terms, tgt_ptr, n_targets, nullptr, out);
}

extern "C" int
acm_gpu_templates_create (ACMPlan *plan, const ACMTemplateSpec *spec, ACMTemplates **out) {
  if (!plan || !out || acm_templates_check (spec, plan->class_sym_bytes ? plan->class_sym_bytes : plan->text_sym_bytes, plan->covered_keywords))
    return ACM_GPU_E_ARG;
  ACMTemplates *made = new (std::nothrow) ACMTemplates ();
  if (!made)
    return ACM_GPU_E_NOMEM;
  if (const int rc = set_create (plan, spec->spell_data, spec->spell_off, spec->k, spec->terms, spec->tgt_ptr, spec->n_templates, spec, &made->set)) {
    delete made;
    return rc;
  }
  *out = made;
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_templates_destroy (ACMTemplates *templates) {
  if (!templates)
    return;
  acm_gpu_approx_destroy (templates->set);
  delete templates;
}

extern "C" int
acm_gpu_templates_info (const ACMTemplates *templates, ACMTemplatesInfo *info) {
  if (!templates || !info)
    return ACM_GPU_E_ARG;
  const ACMApprox *set = templates->set;
  *info = ACMTemplatesInfo{ set->n_targets, set->n_terms, set->n_classes, set->seed_keywords, set->longest, set->max_k, set->max_postings };
  return ACM_GPU_OK;
}

extern "C" void
acm_gpu_approx_destroy (ACMApprox *approx) {
  set_destroy (approx);
}

extern "C" int
acm_gpu_approx_info (const ACMApprox *approx, ACMApproxInfo *info) {
  if (!approx || !info)
    return ACM_GPU_E_ARG;
  *info = ACMApproxInfo{ approx->n_targets, approx->n_terms, approx->seed_keywords, approx->longest, approx->max_k, approx->max_postings };
  return ACM_GPU_OK;
}

extern "C" size_t
acm_gpu_approx_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t n_or_capacity, uint64_t out_capacity, uint64_t n_texts) {
  (void)n_texts; /* (nothing here is sized by the number of texts: the text of a match is a bisection of offsets[]) */
  return set_tmp_bytes (Metric::Mismatches, plan, approx, n_or_capacity, out_capacity);
}

extern "C" size_t
acm_gpu_edit_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t n_or_capacity, uint64_t out_capacity, uint64_t n_texts) {
  (void)n_texts;
  return set_tmp_bytes (Metric::Edits, plan, approx, n_or_capacity, out_capacity);
}

namespace {
/* (d_text and d_dist: what these joins take beside a JoinCall) */
int
set_records_device (Metric metric, const JoinCall &C, const ACMApprox *approx, const void *d_text, uint32_t *d_dist) {
  ACMPlan *plan = C.plan;
  const uint64_t n = C.n, n_symbols = C.n_symbols, n_texts = C.n_texts, out_capacity = C.out_capacity;
  if (!set_usable (metric, plan, approx) || !join_args_ok (C, approx) || (n_symbols && !d_text) || !symbols_ok (d_text, n_symbols, approx->sym_bytes))
    return ACM_GPU_E_ARG;
  hipStream_t st = static_cast<hipStream_t> (C.stream);
  if (n == 0) /* (no record: no match, whatever *d_n says) */
    return no_record (plan, nullptr, C.d_count, st);
  Carve carve (C.d_tmp);
  ApproxK K{};
  const ApproxRoom L = set_carve (metric, carve, n, out_capacity, K);
  if (C.tmp_bytes < carve.total ())
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (plan->device));
  const uint64_t longest = approx->longest + (metric == Metric::Edits ? approx->max_k : 0); /* (a match within k edits may be longer than its target) */
  K.post_ptr = approx->d_post_ptr;
  K.post = approx->d_post;
  K.target = approx->d_target;
  K.spell_off = approx->d_spell_off;
  K.terms = approx->d_terms;
  K.spell = approx->d_spell;
  K.cells = approx->d_cells;
  K.cls_bitmap = approx->d_cls_bitmap;
  K.cls_ptr = approx->d_cls_ptr;
  K.cls_ranges = approx->d_cls_ranges;
  K.cls_flags = approx->d_cls_flags;
  K.n_keywords = approx->n_keywords;
  K.longest = (uint32_t)longest;
  K.tgt_bits = bits_of (approx->n_targets ? approx->n_targets - 1 : 0);
  K.text = d_text;
  K.dist = d_dist;
  bind_join (K, C);
  HIP_TRY (hipMemsetAsync (K.ctl, 0, sizeof (JoinCtl), st));
  int rc = ACM_GPU_E_INTERNAL;
  switch (approx->sym_bytes) {
  case 1: rc = set_passes<uint8_t> (metric, approx->max_k, plan, K, L, n, n_texts, st); break;
  case 2: rc = set_passes<uint16_t> (metric, approx->max_k, plan, K, L, n, n_texts, st); break;
  case 4: rc = set_passes<uint32_t> (metric, approx->max_k, plan, K, L, n, n_texts, st); break;
  case 8: rc = set_passes<uint64_t> (metric, approx->max_k, plan, K, L, n, n_texts, st); break;
  }
  if (rc || !out_capacity)
    return rc;
  /* 5. the order (the kernels return at once when the total does not fit) */
  const dim3 grid = capped_grid (plan, (out_capacity + APPROX_THREADS - 1) / APPROX_THREADS);
  size_t sort_bytes = L.sort_bytes;
  K.key = L.key_a;
  K.idx = L.idx_a;
  HIP_TRY (launch (approx_key1_kernel, grid, dim3 (APPROX_THREADS), 0, st, K));
  HIP_TRY (hipcub::DeviceRadixSort::SortPairs (L.sort, sort_bytes, static_cast<const uint64_t *> (L.key_a), L.key_b, static_cast<const uint32_t *> (L.idx_a),
                                               L.idx_b, (int)out_capacity, 0, (int)(K.tgt_bits + bits_of (longest)), st));
  K.idx_from = L.idx_b;
  HIP_TRY (launch (approx_key2_kernel, grid, dim3 (APPROX_THREADS), 0, st, K));
  sort_bytes = L.sort_bytes;
  HIP_TRY (hipcub::DeviceRadixSort::SortPairs (L.sort, sort_bytes, static_cast<const uint64_t *> (L.key_a), L.key_b, static_cast<const uint32_t *> (L.idx_b),
                                               L.idx_a, (int)out_capacity, 0, (int)bits_of (n_symbols), st));
  K.idx_from = L.idx_a;
  HIP_TRY (launch (approx_gather_kernel, grid, dim3 (APPROX_THREADS), 0, st, K));
  return ACM_GPU_OK;
}

size_t
scan_set_tmp_bytes (Metric metric, const ACMPlan *plan, const ACMApprox *approx, uint64_t capacity, uint64_t out_capacity, uint64_t n_symbols) {
  if (!set_usable (metric, plan, approx) || capacity >= (1ull << 31) || out_capacity >= (1ull << 31))
    return 0;
  Carve c;
  scan_room_carve (c, plan, set_tmp_bytes (metric, plan, approx, capacity, out_capacity), capacity, n_symbols);
  return c.total ();
}

int
scan_set_device (Metric metric, const ScanJoinCall &C, const ACMApprox *approx, uint32_t *d_dist) {
  return scan_then_join (C, set_usable (metric, C.plan, approx), set_tmp_bytes (metric, C.plan, approx, C.capacity, C.out_capacity),
                         [&] (const JoinCall &J) { return set_records_device (metric, J, approx, C.d_text, d_dist); });
}

int
scan_set_host (Metric metric, const ScanJoinHost &H, const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms,
               const uint64_t *tgt_ptr, uint64_t n_targets, const ACMTemplateSpec *tpl) {
  ACMPlan *plan = H.plan;
  return scan_join_host<ACMApprox> (
    H, true,
    [&] (ACMApprox **made) {
      if (metric == Metric::Edits && acm_edit_check (spell_off, k, terms, tgt_ptr, n_targets, plan->covered_keywords)) /* (the set would be made, and refused) */
        return (int)ACM_GPU_E_ARG;
      if (tpl && acm_templates_check (tpl, plan->class_sym_bytes ? plan->class_sym_bytes : plan->text_sym_bytes, plan->covered_keywords))
        return (int)ACM_GPU_E_ARG;
      return set_create (plan, spell_data, spell_off, k, terms, tgt_ptr, n_targets, tpl, made);
    },
    [] (const ACMApprox *, uint64_t) { return true; },
    [&] (const ACMApprox *set, uint64_t capacity) { return scan_set_tmp_bytes (metric, plan, set, capacity, H.out_capacity, H.n_symbols); },
    [&] (const ACMApprox *set, const ScanJoinCall &C, uint32_t *d_dist) { return scan_set_device (metric, C, set, d_dist); });
}
} // namespace

/* the entry points of the two metrics (include/acm_gpu.h) */
extern "C" int
acm_gpu_approx_records_device (ACMPlan *plan, const ACMApprox *approx, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, const void *d_text,
                               uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts, ACMRecord *d_out, uint32_t *d_dist,
                               uint64_t out_capacity, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  return set_records_device (Metric::Mismatches,
                             JoinCall{ plan, d_records, n, d_n, n_symbols, pos_base, d_offsets, n_texts, d_out, out_capacity, d_count, d_tmp, tmp_bytes, stream }, approx,
                             d_text, d_dist);
}

extern "C" int
acm_gpu_edit_records_device (ACMPlan *plan, const ACMApprox *approx, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n, const void *d_text,
                             uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts, ACMRecord *d_out, uint32_t *d_dist,
                             uint64_t out_capacity, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  return set_records_device (Metric::Edits, JoinCall{ plan, d_records, n, d_n, n_symbols, pos_base, d_offsets, n_texts, d_out, out_capacity, d_count, d_tmp, tmp_bytes, stream },
                             approx, d_text, d_dist);
}

/* TEMPLATES: the entry points of APPROX over a template set */
extern "C" size_t
acm_gpu_templates_tmp_bytes (const ACMPlan *plan, const ACMTemplates *templates, uint64_t n_or_capacity, uint64_t out_capacity, uint64_t n_texts) {
  (void)n_texts;
  return templates ? set_tmp_bytes (Metric::Templates, plan, templates->set, n_or_capacity, out_capacity) : 0;
}

extern "C" int
acm_gpu_templates_records_device (ACMPlan *plan, const ACMTemplates *templates, const ACMRecord *d_records, uint64_t n, const uint64_t *d_n,
                                  const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets, uint64_t n_texts, ACMRecord *d_out,
                                  uint32_t *d_dist, uint64_t out_capacity, uint64_t *d_count, void *d_tmp, size_t tmp_bytes, void *stream) {
  return set_records_device (Metric::Templates,
                             JoinCall{ plan, d_records, n, d_n, n_symbols, pos_base, d_offsets, n_texts, d_out, out_capacity, d_count, d_tmp, tmp_bytes, stream },
                             templates ? templates->set : nullptr, d_text, d_dist);
}

extern "C" size_t
acm_gpu_scan_templates_tmp_bytes (const ACMPlan *plan, const ACMTemplates *templates, uint64_t capacity, uint64_t out_capacity, uint64_t n_symbols,
                                  uint64_t n_texts) {
  (void)n_texts;
  return templates ? scan_set_tmp_bytes (Metric::Templates, plan, templates->set, capacity, out_capacity, n_symbols) : 0;
}

extern "C" int
acm_gpu_scan_templates_device (ACMPlan *plan, const ACMTemplates *templates, const void *d_text, uint64_t n_symbols, uint64_t pos_base,
                               const uint64_t *d_offsets, uint64_t n_texts, uint64_t capacity, ACMRecord *d_out, uint32_t *d_dist, uint64_t out_capacity,
                               uint64_t *d_count, uint64_t *d_found, void *d_tmp, size_t tmp_bytes, void *stream) {
  return scan_set_device (Metric::Templates,
                          ScanJoinCall{ plan, d_text, n_symbols, pos_base, d_offsets, n_texts, capacity, d_out, out_capacity, d_count, d_found, d_tmp, tmp_bytes, stream },
                          templates ? templates->set : nullptr, d_dist);
}

extern "C" int
acm_gpu_scan_templates_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                             const ACMTemplateSpec *spec, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  if (!spec)
    return ACM_GPU_E_ARG;
  return scan_set_host (Metric::Templates, ScanJoinHost{ plan, text, n_symbols, pos_base, offsets, n_texts, out, dist, out_capacity, n_found }, spec->spell_data, spec->spell_off,
                        spec->k, spec->terms, spec->tgt_ptr, spec->n_templates, spec);
}

extern "C" size_t
acm_gpu_scan_approx_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t capacity, uint64_t out_capacity, uint64_t n_symbols, uint64_t n_texts) {
  (void)n_texts;
  return scan_set_tmp_bytes (Metric::Mismatches, plan, approx, capacity, out_capacity, n_symbols);
}

extern "C" size_t
acm_gpu_scan_edit_tmp_bytes (const ACMPlan *plan, const ACMApprox *approx, uint64_t capacity, uint64_t out_capacity, uint64_t n_symbols, uint64_t n_texts) {
  (void)n_texts;
  return scan_set_tmp_bytes (Metric::Edits, plan, approx, capacity, out_capacity, n_symbols);
}

extern "C" int
acm_gpu_scan_approx_device (ACMPlan *plan, const ACMApprox *approx, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets,
                            uint64_t n_texts, uint64_t capacity, ACMRecord *d_out, uint32_t *d_dist, uint64_t out_capacity, uint64_t *d_count,
                            uint64_t *d_found, void *d_tmp, size_t tmp_bytes, void *stream) {
  return scan_set_device (Metric::Mismatches,
                          ScanJoinCall{ plan, d_text, n_symbols, pos_base, d_offsets, n_texts, capacity, d_out, out_capacity, d_count, d_found, d_tmp, tmp_bytes, stream }, approx,
                          d_dist);
}

extern "C" int
acm_gpu_scan_edit_device (ACMPlan *plan, const ACMApprox *approx, const void *d_text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *d_offsets,
                          uint64_t n_texts, uint64_t capacity, ACMRecord *d_out, uint32_t *d_dist, uint64_t out_capacity, uint64_t *d_count,
                          uint64_t *d_found, void *d_tmp, size_t tmp_bytes, void *stream) {
  return scan_set_device (Metric::Edits, ScanJoinCall{ plan, d_text, n_symbols, pos_base, d_offsets, n_texts, capacity, d_out, out_capacity, d_count, d_found, d_tmp, tmp_bytes, stream },
                          approx, d_dist);
}

extern "C" int
acm_gpu_scan_approx_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                          const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr,
                          uint64_t n_targets, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  return scan_set_host (Metric::Mismatches, ScanJoinHost{ plan, text, n_symbols, pos_base, offsets, n_texts, out, dist, out_capacity, n_found }, spell_data, spell_off, k, terms,
                        tgt_ptr, n_targets, nullptr);
}

extern "C" int
acm_gpu_scan_edit_host (ACMPlan *plan, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                        const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr,
                        uint64_t n_targets, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  return scan_set_host (Metric::Edits, ScanJoinHost{ plan, text, n_symbols, pos_base, offsets, n_texts, out, dist, out_capacity, n_found }, spell_data, spell_off, k, terms, tgt_ptr,
                        n_targets, nullptr);
}

/* ------------------------------------------------------------------ records on the wire (include/acm_gpu.h) */
extern "C" int
acm_gpu_wire_bits (const ACMPlan *plan, uint64_t span, uint32_t *pos_bits, uint32_t *len_bits, uint32_t *kw_bits) {
  if (!plan || !pos_bits || !len_bits || !kw_bits)
    return ACM_GPU_E_ARG;
  auto bits = [] (uint64_t v) { /* bits that hold every value in [0, v] */
    uint32_t b = 1;
    while (b < 64 && (v >> b))
      b++;
    return b;
  };
  const uint64_t kw_max = (uint64_t)plan->covered_keywords + plan->finfo.n_keywords + plan->kw_base; /* (an upper bound: a delta's ids follow the plan's) */
  *pos_bits = bits (span ? span - 1 : 0);
  *len_bits = bits (plan_lmax (plan));
  *kw_bits = bits (kw_max);
  return *pos_bits + *len_bits + *kw_bits <= 64 ? ACM_GPU_OK : ACM_GPU_E_INELIGIBLE;
}

extern "C" int
acm_gpu_pack_records_device (const ACMRecord *d_records, uint64_t n, uint64_t pos_lo, uint32_t pos_bits, uint32_t len_bits, uint64_t *d_packed,
                             void *stream) {
  if ((n && (!d_records || !d_packed)) || pos_bits == 0 || pos_bits + len_bits >= 64)
    return ACM_GPU_E_ARG;
  if (n == 0)
    return ACM_GPU_OK;
  const uint64_t blocks = (n + 255) / 256;
  HIP_TRY (launch (pack_records_kernel, dim3 ((uint32_t)(blocks < 16384 ? blocks : 16384)), dim3 (256), 0, static_cast<hipStream_t> (stream), d_records, n,
                   pos_lo, pos_bits, len_bits, d_packed));
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_unpack_records_device (const uint64_t *d_packed, uint64_t n, uint64_t pos_lo, uint32_t pos_bits, uint32_t len_bits, ACMRecord *d_records,
                               void *stream) {
  if ((n && (!d_records || !d_packed)) || pos_bits == 0 || pos_bits + len_bits >= 64)
    return ACM_GPU_E_ARG;
  if (n == 0)
    return ACM_GPU_OK;
  const uint64_t blocks = (n + 255) / 256;
  HIP_TRY (launch (unpack_records_kernel, dim3 ((uint32_t)(blocks < 16384 ? blocks : 16384)), dim3 (256), 0, static_cast<hipStream_t> (stream), d_packed, n,
                   pos_lo, pos_bits, len_bits, d_records));
  return ACM_GPU_OK;
}

/* ------------------------------------------------------------------ several GPUs, one process (include/acm_gpu.h)
 * contiguous shards, an lmax - 1 halo, tables replicated, no collective on the data
 * path; the one exchange step is the gather of the ordered records on devices[0] by direct peer
 * copies (reference model: one shared machine, one cursor per worker, README.md:364). */
struct ACMMulti {
  std::vector<int> dev;        /* per shard */
  std::vector<int> distinct;   /* the devices in use, devices[0] first */
  std::vector<ACMPlan *> plan; /* per distinct device */
  std::vector<hipStream_t> stream;
  uint32_t lmax = 0, sym_bytes = 1;
  /* what a shard's scan needs on its device, kept from call to call (grow-only): hipMalloc and
   * hipFree wait for the device, and a scan of config 4 wants 7 GB of records + twice that of
   * scratch per shard -- allocated once, sized by what the call before found */
  struct ShardBuf {
    ACMRecord *rec = nullptr;
    uint64_t rec_cap = 0;
    uint64_t *cnt = nullptr;
    void *tmp = nullptr;
    size_t tmp_cap = 0;
    uint64_t last_found = 0, last_span = 0;
  };
  std::vector<ShardBuf> buf; /* per shard */
  uint64_t *h_found = nullptr; /* pinned, one count per shard */
  /* records on the wire: a shard of another device packs its ordered records to 8 bytes each
   * (acm_gpu_pack_records_device), sends them to this staging area on devices[0], and they are
   * unpacked into their place there -- half the bytes over the shard's one link to the root */
  uint64_t *stage0 = nullptr;
  uint64_t stage0_cap = 0; /* in 8-byte words */
  std::vector<hipEvent_t> arrived; /* per shard: its packed records have landed on devices[0] */
  int slot_of (int device) const {
    for (size_t i = 0; i < distinct.size (); i++)
      if (distinct[i] == device)
        return (int)i;
    return -1;
  }
};

extern "C" void
acm_gpu_multi_destroy (ACMMulti *mu) {
  if (!mu)
    return;
  for (size_t i = 0; i < mu->distinct.size (); i++) {
    (void)hipSetDevice (mu->distinct[i]);
    if (i < mu->stream.size () && mu->stream[i]) {
      (void)hipStreamSynchronize (mu->stream[i]);
      (void)hipStreamDestroy (mu->stream[i]);
    }
    if (i < mu->plan.size () && mu->plan[i])
      acm_gpu_plan_destroy (mu->plan[i]);
  }
  for (size_t r = 0; r < mu->buf.size (); r++) {
    (void)hipSetDevice (mu->dev[r]);
    if (mu->buf[r].rec) (void)hipFree (mu->buf[r].rec);
    if (mu->buf[r].cnt) (void)hipFree (mu->buf[r].cnt);
    if (mu->buf[r].tmp) (void)hipFree (mu->buf[r].tmp);
  }
  if (mu->h_found)
    (void)hipHostFree (mu->h_found);
  if (mu->stage0) {
    (void)hipSetDevice (mu->dev[0]);
    (void)hipFree (mu->stage0);
  }
  for (size_t r = 0; r < mu->arrived.size (); r++)
    if (mu->arrived[r]) {
      (void)hipSetDevice (mu->dev[r]);
      (void)hipEventDestroy (mu->arrived[r]);
    }
  delete mu;
}

extern "C" int
acm_gpu_multi_create (ACMachine *machine, const int *devices, int n_shards, ACMMulti **out) {
  if (!machine || !devices || n_shards < 1 || !out)
    return ACM_GPU_E_ARG;
  int ndev = 0;
  if (hipGetDeviceCount (&ndev) != hipSuccess || ndev <= 0)
    return ACM_GPU_E_NODEVICE;
  ACMMulti *mu = new (std::nothrow) ACMMulti ();
  if (!mu)
    return ACM_GPU_E_NOMEM;
  for (int r = 0; r < n_shards; r++) {
    if (devices[r] < 0 || devices[r] >= ndev) {
      delete mu;
      return ACM_GPU_E_ARG;
    }
    mu->dev.push_back (devices[r]);
    if (mu->slot_of (devices[r]) < 0)
      mu->distinct.push_back (devices[r]);
  }
  /* one snapshot of the dictionary for every device: the same tables everywhere */
  ACMFlat *flat = nullptr;
  int rc = acm_flatten (machine, &flat);
  if (rc) {
    delete mu;
    return rc;
  }
  ACMFlatInfo fi;
  acm_flat_info (flat, &fi);
  mu->lmax = fi.lmax;
  mu->sym_bytes = fi.sym_bytes;
  mu->plan.assign (mu->distinct.size (), nullptr);
  mu->stream.assign (mu->distinct.size (), nullptr);
  mu->buf.assign (mu->dev.size (), ACMMulti::ShardBuf ());
  if (hipHostMalloc (reinterpret_cast<void **> (&mu->h_found), mu->dev.size () * sizeof (uint64_t), hipHostMallocDefault) != hipSuccess) {
    mu->h_found = nullptr;
    acm_flat_release (flat);
    delete mu;
    return ACM_GPU_E_NOMEM;
  }
  for (size_t i = 0; i < mu->distinct.size () && !rc; i++) {
    rc = acm_gpu_plan_create_flat (flat, mu->distinct[i], &mu->plan[i]);
    if (!rc && (hipSetDevice (mu->distinct[i]) != hipSuccess || hipStreamCreateWithFlags (&mu->stream[i], hipStreamNonBlocking) != hipSuccess))
      rc = ACM_GPU_E_HIP;
    /* direct peer copies into devices[0] where the hardware offers them (otherwise the runtime stages the copy) */
    if (!rc && i > 0) {
      int can = 0;
      if (hipDeviceCanAccessPeer (&can, mu->distinct[i], mu->distinct[0]) == hipSuccess && can) {
        const hipError_t e = hipDeviceEnablePeerAccess (mu->distinct[0], 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
          (void)hipGetLastError ();
      }
    }
  }
  acm_flat_release (flat);
  if (rc) {
    acm_gpu_multi_destroy (mu);
    return rc;
  }
  *out = mu;
  return ACM_GPU_OK;
}

extern "C" int
acm_gpu_multi_shard_bounds (const ACMMulti *mu, uint64_t n, int shard, uint64_t *read_begin, uint64_t *own_begin, uint64_t *own_end) {
  if (!mu || shard < 0 || shard >= (int)mu->dev.size ())
    return ACM_GPU_E_ARG;
  const uint64_t R = mu->dev.size ();
  /* the rule of sharded.shard_bounds (rank r owns [r N / R, (r + 1) N / R)), with the halo grown to
   * the next 16-byte boundary of the text so that a shard's buffer can keep the text's alignment */
  const uint64_t b = n / R * (uint64_t)shard + n % R * (uint64_t)shard / R, e = n / R * (uint64_t)(shard + 1) + n % R * (uint64_t)(shard + 1) / R;
  const uint64_t per16 = 16 / mu->sym_bytes ? 16 / mu->sym_bytes : 1;
  const uint64_t warm = mu->lmax > 1 ? mu->lmax - 1 : 0;
  uint64_t rb = b > warm ? b - warm : 0;
  rb = rb / per16 * per16;
  if (read_begin)
    *read_begin = rb;
  if (own_begin)
    *own_begin = b;
  if (own_end)
    *own_end = e;
  return ACM_GPU_OK;
}

namespace {
/* waits for the stream of every device in use: all of them, whatever fails; the first failure */
hipError_t
drain (ACMMulti *mu) {
  hipError_t first = hipSuccess;
  for (size_t i = 0; i < mu->distinct.size (); i++) {
    hipError_t e = hipSetDevice (mu->distinct[i]);
    if (e == hipSuccess)
      e = hipStreamSynchronize (mu->stream[i]);
    if (first == hipSuccess)
      first = e;
  }
  return first;
}

/* a device buffer kept from call to call, of at least `want` units (grow-only; *cap counts units) */
template <typename T, typename N>
hipError_t
grow_to (T **buf, N *cap, N want, size_t unit_bytes) {
  if (*cap >= want)
    return hipSuccess;
  if (*buf)
    (void)hipFree (*buf);
  *buf = nullptr;
  *cap = 0;
  const hipError_t e = hipMalloc (reinterpret_cast<void **> (buf), want * unit_bytes);
  if (e == hipSuccess)
    *cap = want;
  return e;
}

/* shards scanned, ordered and gathered: d_text[r] on dev[r] holds [read_begin_r, own_end_r) */
int
multi_scan (ACMMulti *mu, const void *const *d_text, uint64_t n, ACMRecord *d_out, uint64_t capacity, uint64_t *n_found) {
  const size_t R = mu->dev.size ();
  struct Shard {
    uint64_t rb = 0, b = 0, e = 0;
    int slot = 0;
  };
  std::vector<Shard> sh (R);
  int rc = ACM_GPU_OK;
#define MULTI_TRY(expr)                                                                            \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      fprintf (stderr, "acm_gpu: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString (_e), __FILE__, __LINE__); \
      (void)drain (mu);                                                                            \
      return _e == hipErrorOutOfMemory ? ACM_GPU_E_NOMEM : ACM_GPU_E_HIP;                          \
    }                                                                                              \
  } while (0)
  /* a shard's record buffer and scratch: at least `want` records (grow-only, kept by the handle) */
  auto ensure = [&] (size_t r, uint64_t want) -> int {
    ACMMulti::ShardBuf &B = mu->buf[r];
    const Shard &s = sh[r];
    if (!B.cnt && hipMalloc (reinterpret_cast<void **> (&B.cnt), 8) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    if (grow_to (&B.rec, &B.rec_cap, want, sizeof (ACMRecord)) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    const size_t tb = s.e > s.b ? acm_gpu_scan_ordered_tmp_bytes (mu->plan[s.slot], B.rec_cap, s.e - s.rb) : 0;
    if (grow_to (&B.tmp, &B.tmp_cap, tb, 1) != hipSuccess)
      return ACM_GPU_E_NOMEM;
    return ACM_GPU_OK;
  };
  /* first pass: every shard into a record buffer sized by what the call before found on a text of
   * this length (+ an eighth), or by a guess (one match per 32 symbols); the counts tell which
   * shards need a second pass with the exact size */
  for (int pass = 0; pass < 2; pass++) {
    bool any = false;
    for (size_t r = 0; r < R; r++) {
      Shard &s = sh[r];
      ACMMulti::ShardBuf &B = mu->buf[r];
      if (pass == 0) {
        s.slot = mu->slot_of (mu->dev[r]);
        (void)acm_gpu_multi_shard_bounds (mu, n, (int)r, &s.rb, &s.b, &s.e);
      } else if (mu->h_found[r] <= B.rec_cap)
        continue; /* the first pass had room for everything it found */
      any = true;
      MULTI_TRY (hipSetDevice (mu->dev[r]));
      uint64_t want = mu->h_found[r];
      if (pass == 0) {
        const uint64_t span = s.e - s.b;
        want = B.last_found && B.last_span == span ? B.last_found + B.last_found / 8 + 4096 : span / 32 + 4096;
        if (want < B.rec_cap)
          want = B.rec_cap;
      }
      rc = ensure (r, want);
      if (rc) {
        (void)drain (mu);
        return rc;
      }
      /* (shards of one device share its stream: their scans run one after the other.)  Scan and
       * canonical order in one call: nothing waits for the host between them, and 4-gram plans scan
       * in tiles and order in one pass */
      if (s.e > s.b) {
        rc = acm_gpu_scan_ordered_device (mu->plan[s.slot], d_text[r], s.e - s.rb, s.b - s.rb, s.rb, B.rec, B.rec_cap, B.cnt, B.tmp, B.tmp_cap, mu->stream[s.slot]);
        if (rc) {
          (void)drain (mu);
          return rc;
        }
      } else
        MULTI_TRY (hipMemsetAsync (B.cnt, 0, 8, mu->stream[s.slot]));
      MULTI_TRY (hipMemcpyAsync (&mu->h_found[r], B.cnt, 8, hipMemcpyDeviceToHost, mu->stream[s.slot]));
    }
    if (!any)
      break;
    MULTI_TRY (drain (mu));
  }
  uint64_t total = 0;
  for (size_t r = 0; r < R; r++) {
    total += mu->h_found[r];
    mu->buf[r].last_found = mu->h_found[r];
    mu->buf[r].last_span = sh[r].e - sh[r].b;
  }
  *n_found = total;
  if (total > capacity)
    return ACM_GPU_E_OVERFLOW;
  /* (every shard's records are in canonical order where they are:) each shard's run into its place
   * on devices[0] -- from another device as 8-byte words when the fields fit (acm_gpu_wire_bits):
   * packed into the shard's scratch, sent to the staging area, unpacked there behind an event */
  const char *wire_env = getenv ("ACM_GPU_WIRE"); /* 0: 16-byte records over the links; 2: the wire form for shards of devices[0] too (tests on one GPU) */
  const bool wire_off = wire_env && atoi (wire_env) == 0, wire_all = wire_env && atoi (wire_env) == 2;
  uint64_t remote = 0;
  for (size_t r = 0; r < R; r++)
    if (mu->dev[r] != mu->dev[0] || wire_all)
      remote += mu->h_found[r];
  if (remote > mu->stage0_cap && !wire_off) {
    MULTI_TRY (hipSetDevice (mu->dev[0]));
    MULTI_TRY (grow_to (&mu->stage0, &mu->stage0_cap, remote, 8));
  }
  if (mu->arrived.size () < R)
    mu->arrived.resize (R, nullptr);
  uint64_t off = 0, soff = 0;
  for (size_t r = 0; r < R; r++) {
    const Shard &s = sh[r];
    const uint64_t found = mu->h_found[r];
    MULTI_TRY (hipSetDevice (mu->dev[r]));
    hipStream_t st = mu->stream[s.slot];
    if (found) {
      uint32_t pb = 0, lb = 0, kb = 0;
      if (mu->dev[r] == mu->dev[0] && !wire_all)
        MULTI_TRY (hipMemcpyAsync (d_out + off, mu->buf[r].rec, found * sizeof (ACMRecord), hipMemcpyDeviceToDevice, st));
      else if (!wire_off && acm_gpu_wire_bits (mu->plan[s.slot], s.e - s.rb, &pb, &lb, &kb) == ACM_GPU_OK && found * 8 <= mu->buf[r].tmp_cap) {
        uint64_t *packed = static_cast<uint64_t *> (mu->buf[r].tmp); /* (the scan's scratch: it is done with it) */
        rc = acm_gpu_pack_records_device (mu->buf[r].rec, found, s.rb, pb, lb, packed, st);
        if (!rc) {
          MULTI_TRY (hipMemcpyPeerAsync (mu->stage0 + soff, mu->dev[0], packed, mu->dev[r], found * 8, st));
          if (!mu->arrived[r])
            MULTI_TRY (hipEventCreateWithFlags (&mu->arrived[r], hipEventDisableTiming));
          MULTI_TRY (hipEventRecord (mu->arrived[r], st));
          MULTI_TRY (hipSetDevice (mu->dev[0]));
          MULTI_TRY (hipStreamWaitEvent (mu->stream[0], mu->arrived[r], 0));
          rc = acm_gpu_unpack_records_device (mu->stage0 + soff, found, s.rb, pb, lb, d_out + off, mu->stream[0]);
        }
        if (rc) {
          (void)drain (mu);
          return rc;
        }
        soff += found;
      } else
        MULTI_TRY (hipMemcpyPeerAsync (d_out + off, mu->dev[0], mu->buf[r].rec, mu->dev[r], found * sizeof (ACMRecord), st));
    }
    off += found;
  }
  MULTI_TRY (drain (mu));
  for (size_t i = 0; i < mu->distinct.size () && !rc; i++)
    rc = acm_gpu_plan_status (mu->plan[i]);
  return rc;
#undef MULTI_TRY
}
} // namespace

extern "C" int
acm_gpu_multi_scan_device (ACMMulti *mu, const void *const *d_shard_text, uint64_t n, ACMRecord *d_records, uint64_t capacity,
                           uint64_t *n_found) {
  if (!mu || !n_found || (n && !d_shard_text) || (capacity && !d_records))
    return ACM_GPU_E_ARG;
  return multi_scan (mu, d_shard_text, n, d_records, capacity, n_found);
}

extern "C" int
acm_gpu_multi_scan_host (ACMMulti *mu, const void *text, uint64_t n, ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  if (!mu || !n_found || (n && !text) || (capacity && !records))
    return ACM_GPU_E_ARG;
  const size_t R = mu->dev.size ();
  std::vector<void *> d_text (R, nullptr);
  ACMRecord *d_out = nullptr;
  int rc = ACM_GPU_OK;
  auto cleanup = [&] () {
    for (size_t r = 0; r < R; r++)
      if (d_text[r]) {
        (void)hipSetDevice (mu->dev[r]);
        (void)hipFree (d_text[r]);
      }
    if (d_out) {
      (void)hipSetDevice (mu->dev[0]);
      (void)hipFree (d_out);
    }
  };
  for (size_t r = 0; r < R && !rc; r++) {
    uint64_t rb, b, e;
    (void)acm_gpu_multi_shard_bounds (mu, n, (int)r, &rb, &b, &e);
    const size_t bytes = (size_t)(e - rb) * mu->sym_bytes;
    const int slot = mu->slot_of (mu->dev[r]);
    if (hipSetDevice (mu->dev[r]) != hipSuccess || hipMalloc (&d_text[r], bytes + 16) != hipSuccess)
      rc = ACM_GPU_E_NOMEM;
    else if (bytes && hipMemcpyAsync (d_text[r], static_cast<const unsigned char *> (text) + (size_t)rb * mu->sym_bytes, bytes, hipMemcpyHostToDevice,
                                      mu->stream[slot]) != hipSuccess)
      rc = ACM_GPU_E_HIP;
  }
  if (!rc && (hipSetDevice (mu->dev[0]) != hipSuccess || hipMalloc (reinterpret_cast<void **> (&d_out), (capacity ? capacity : 1) * sizeof (ACMRecord)) != hipSuccess))
    rc = ACM_GPU_E_NOMEM;
  if (!rc)
    rc = multi_scan (mu, d_text.data (), n, d_out, capacity, n_found);
  if (!rc && *n_found) {
    if (hipSetDevice (mu->dev[0]) != hipSuccess || hipMemcpy (records, d_out, *n_found * sizeof (ACMRecord), hipMemcpyDeviceToHost) != hipSuccess)
      rc = ACM_GPU_E_HIP;
  }
  cleanup ();
  return rc;
}

/* the reference's dictionaries grow while they are used (README.md:352-356,
 * generic_test.c:214-229).  Brings `plan` up to date with `machine` (the machine it was made from,
 * later): plans of the start-parallel kernel take the new keywords as edits of a few table words
 * (StartsMirror); every other plan keeps its tables and gets the new keywords as a small delta
 * plan scanned beside it (below), merged into one plan again only now and then. */
extern "C" int
acm_gpu_plan_update (ACMPlan *plan, ACMachine *machine) {
  if (!plan || !machine)
    return ACM_GPU_E_ARG;
  const uint64_t gen = acm_internal_generation (machine);
  uint32_t sym_bytes = 0;
  const bool plain = acm_internal_symbol_bytes (machine, &sym_bytes) == ACM_GPU_OK;
  if (plan->kind == PlanKind::Starts && plan->mir && plain && !plan->class_sym_bytes && sym_bytes == plan->finfo.sym_bytes) {
    StartsMirror &M = *plan->mir;
    acm_internal_lock (machine);
    const uint32_t nk = (uint32_t)acm_nb_keywords (machine);
    if (nk < M.n_keywords) {
      acm_internal_unlock (machine);
      return ACM_GPU_E_ARG; /* not the machine this plan came from */
    }
    MatchHolder h;
    acm_matcher_init (&h);
    std::vector<uint32_t> sym;
    int rc = ACM_GPU_OK;
    for (uint32_t k = M.n_keywords; k < nk && rc == ACM_GPU_OK; k++) {
      rc = acm_internal_get_keyword (machine, k, &h); /* the machine lock is held */
      if (rc)
        break;
      sym.resize (h.length);
      for (size_t i = 0; i < h.length; i++) {
        const unsigned char *l = static_cast<const unsigned char *> (h.letters[i]);
        uint32_t v = 0;
        for (uint32_t bb = 0; bb < sym_bytes; bb++)
          v |= (uint32_t)l[bb] << (8 * bb);
        sym[i] = v;
      }
      if (M.n_states + h.length >= ST_STATE)
        rc = ACM_GPU_E_INELIGIBLE;
      else
        mirror_insert (M, sym.data (), (uint32_t)h.length, k);
    }
    acm_matcher_release (&h);
    acm_internal_unlock (machine);
    if (rc)
      return rc;
    plan->finfo.n_states = M.n_states;
    plan->finfo.n_edges = M.n_edges;
    plan->finfo.n_keywords = M.n_keywords;
    plan->covered_keywords = M.n_keywords;
    plan->finfo.lmax = M.lmax;
    plan->generation = gen;
    return ACM_GPU_OK;
  }
  /* Every other kind of plan has tables that are functions of the whole dictionary (a new keyword
   * changes a column of up to every failure-resolved row, the rank of every later 4-gram ...).
   * They are left alone: the keywords the machine got since the plan was made go into a small
   * delta plan of their own, rebuilt from just those keywords at every update -- a cost that does
   * not depend on the size of the dictionary -- and scanned after the plan itself (scan_plan).
   * Only when the delta has grown past an eighth of the dictionary (at least 256 keywords) is
   * everything rebuilt into one plan again.  (`gen` was read before the snapshots: keywords
   * inserted while they are taken leave the plan stale, never wrongly fresh.) */
  HIP_TRY (hipSetDevice (plan->device));
  for (size_t i = 0; i < plan->retired.size ();) { /* deltas no scan can be using any more */
    ACMPlan::Retired &r = plan->retired[i];
    if (r.done && hipEventQuery (r.done) == hipSuccess) {
      (void)hipEventDestroy (r.done);
      acm_gpu_plan_destroy (r.plan);
      plan->retired.erase (plan->retired.begin () + (long)i);
    } else
      i++;
  }
  const uint32_t base_kw = plan->finfo.n_keywords;
  acm_internal_lock (machine);
  const uint32_t nk = (uint32_t)acm_nb_keywords (machine);
  if (nk < plan->covered_keywords) {
    acm_internal_unlock (machine);
    return ACM_GPU_E_ARG; /* not the machine this plan came from */
  }
  /* A delta is a second pass over every text: on 1 GiB of config 2's text 0.57 ms per scan against
   * 0.32 without one (tools/exp_delta_big.py: a dense delta pass runs at the dense kernel's rate
   * whatever its size), while one plan of everything costs ~3.5 ms per 1,000 keywords once.  So the
   * delta is also given up when the texts scanned with it add up to more than that is worth:
   * 14 Gi symbols per 1,000 keywords of the dictionary (acm_scan asks after every scan). */
  const bool scanned_enough = plan->delta && plan->delta_scanned > (uint64_t)(base_kw > 1000 ? base_kw : 1000) * (14ull << 20);
  if (nk == plan->covered_keywords && !scanned_enough) {
    acm_internal_unlock (machine);
    plan->generation = gen;
    return ACM_GPU_OK;
  }
  const uint32_t threshold = base_kw / 8 > 256 ? base_kw / 8 : 256;
  const char *delta_env = getenv ("ACM_GPU_DELTA"); /* 0: always rebuild (experiments) */
  if (nk - base_kw <= threshold && !scanned_enough && !(delta_env && atoi (delta_env) == 0)) {
    /* the new keywords into a machine of their own: same comparator, the main machine's letters */
    CMP_TYPE cmp;
    void *cmp_arg;
    acm_internal_comparator (machine, &cmp, &cmp_arg);
    ACMachine *tm = acm_create (cmp, cmp_arg, 0);
    MatchHolder h;
    acm_matcher_init (&h);
    int rc = ACM_GPU_OK;
    uint32_t lmax = plan->finfo.lmax;
    for (uint32_t k = base_kw; k < nk && rc == ACM_GPU_OK; k++) {
      rc = acm_internal_get_keyword (machine, k, &h); /* the machine lock is held */
      if (rc)
        break;
      ACState *cur = acm_initiate (tm);
      for (size_t i = 0; i < h.length; i++)
        acm_insert_letter_of_keyword (&cur, const_cast<void *> (h.letters[i]));
      (void)acm_insert_end_of_keyword (&cur, 0, 0);
      if (h.length > lmax)
        lmax = (uint32_t)h.length;
    }
    acm_matcher_release (&h);
    acm_internal_unlock (machine);
    ACMFlat *flat = nullptr;
    if (!rc)
      rc = plan->class_sym_bytes ? acm_flatten_classes (tm, plan->class_sym_bytes, &flat) : acm_flatten (tm, &flat);
    acm_release (tm);
    ACMPlan *fresh = nullptr;
    if (!rc) {
      rc = plan_create (flat, plan->device, base_kw, &fresh);
      acm_flat_release (flat);
    }
    if (rc)
      return rc;
    fresh->class_sym_bytes = plan->class_sym_bytes;
    fresh->cmp32 = plan->cmp32;
    fresh->cmp32_arg = plan->cmp32_arg;
    fresh->segment = plan->segment;
    fresh->shared_items = &plan->items ();
    if (plan->delta)
      plan->retired.push_back (ACMPlan::Retired{ plan->delta, nullptr });
    plan->delta = fresh;
    plan->covered_keywords = nk;
    plan->finfo.lmax = lmax; /* halos and sort keys go by the longest keyword of both */
    plan->generation = gen;
    return ACM_GPU_OK;
  }
  acm_internal_unlock (machine);
  /* the delta has outgrown its share: one plan of everything, behind the same handle */
  ACMPlan *fresh = nullptr;
  int rc = plan->class_sym_bytes ? acm_gpu_plan_create_classes (machine, plan->class_sym_bytes, plan->device, &fresh)
                                 : acm_gpu_plan_create (machine, plan->device, &fresh);
  if (rc)
    return rc;
  HIP_TRY (hipDeviceSynchronize ()); /* scans in flight still read the old tables */
  /* timing goes on across the rebuild: the launches sampled so far into the totals (the device is idle), then the
   * switch, the period, the place in it, the totals and the events themselves move to the new tables */
  rc = acm_gpu_plan_timing_read_all (plan, nullptr, nullptr, nullptr);
  if (rc) {
    acm_gpu_plan_destroy (fresh);
    return rc;
  }
  const uint64_t segment = plan->segment;
  const uint32_t merges = plan->merges + 1;
  std::swap (*plan, *fresh);
  plan->timing = fresh->timing;
  plan->timing_every = fresh->timing_every;
  plan->timing_seq = fresh->timing_seq;
  plan->timing_ms = fresh->timing_ms;
  plan->timing_all_ms = fresh->timing_all_ms;
  plan->timing_launches = fresh->timing_launches;
  std::swap (plan->events, fresh->events);
  plan->events_used = 0;
  acm_gpu_plan_destroy (fresh); /* the old tables, their delta and what was retired */
  plan->segment = segment;
  plan->merges = merges;
  plan->generation = gen;
  return ACM_GPU_OK;
}

namespace {
/* acm_release drops the cached plan through this hook: set once, when the library is loaded */
struct PlanDropperInit {
  PlanDropperInit () { acm_internal_plan_dropper = drop_cached_plan; }
} plan_dropper_init;
} // namespace

/* The reference lets many threads work on one shared machine (README.md:364); the cached plan and
 * its scratch buffers serve one scan at a time, so concurrent acm_scan calls on one machine queue
 * up on the machine's plan lock (threads that want to scan in parallel make a plan each). */
namespace {
/* what acm_scan and acm_scan_batch run on a machine (include/acm_gpu.h) */
struct ScanRoute {
  int path = ACM_SCAN_PATH_NONE; /* ACM_SCAN_PATH_* */
  uint32_t said = 0;             /* the declared symbol size (the host loop's stride) */
  ACMPlan *plan = nullptr;       /* the machine's cached plan, up to date (GPU paths, from route_plan) */
};

/* which path: ACM_CMP_DEFAULT over 1/2/4/8 bytes -> GPU; another comparator with its symbol size
 * declared -> GPU over its classes (1/2/4 bytes) or the caller loop on the host */
int
scan_route (ACMachine *machine, ScanRoute *R) {
  uint32_t own_bytes = 0;
  const bool plain = acm_internal_symbol_bytes (machine, &own_bytes) == ACM_GPU_OK;
  uint32_t said = acm_internal_declared_symbol_bytes (machine);
  CMP_TYPE cmp = nullptr;
  void *cmp_arg = nullptr;
  acm_internal_comparator (machine, &cmp, &cmp_arg);
  /* (ACM_CMP_DEFAULT over symbols of another size says the size itself: memcmp's length) */
  if (!plain && said == 0 && cmp == ACM_CMP_DEFAULT && cmp_arg && *static_cast<const size_t *> (cmp_arg) > 0 &&
      *static_cast<const size_t *> (cmp_arg) <= 4096)
    said = (uint32_t)*static_cast<const size_t *> (cmp_arg);
  if (!plain && said == 0)
    return ACM_GPU_E_INELIGIBLE;
  /* (memcmp over 3, 5, ... bytes: no classes to enumerate, the loop itself) */
  const bool classes = !plain && (said == 1 || said == 2 || said == 4) && cmp != ACM_CMP_DEFAULT;
  R->said = said;
  R->path = plain ? ACM_SCAN_PATH_GPU : classes ? ACM_SCAN_PATH_GPU_CLASSES : ACM_SCAN_PATH_CPU_LOOP;
  return ACM_GPU_OK;
}

/* the GPU paths, with the machine's plan lock held: the cached plan, made or brought up to date.
 * A comparator that is no consistent order over all symbol values (acm_flatten_classes refuses it)
 * cannot be taken by the GPU by its nature: the route becomes the loop itself. */
int
route_plan (ACMachine *machine, ScanRoute *R) {
  const bool classes = R->path == ACM_SCAN_PATH_GPU_CLASSES;
  int rc = ACM_GPU_OK;
  void **slot = acm_internal_plan_slot (machine);
  ACMPlan *plan = static_cast<ACMPlan *> (*slot);
  if (plan && (plan->generation != acm_internal_generation (machine) ||
               (plan->delta && plan->delta_scanned > (uint64_t)(plan->finfo.n_keywords > 1000 ? plan->finfo.n_keywords : 1000) * (14ull << 20))))
    rc = acm_gpu_plan_update (plan, machine); /* new keywords, or a delta that has cost more second passes than one plan of everything */
  if (!rc && !plan) {
    int device = 0;
    if (const char *e = getenv ("ACM_GPU_DEVICE"))
      device = atoi (e);
    /* keywords inserted while the tables are being made are picked up by the next call: the
     * generation is read first */
    const uint64_t gen = acm_internal_generation (machine);
    rc = classes ? acm_gpu_plan_create_classes (machine, R->said, device, &plan) : acm_gpu_plan_create (machine, device, &plan);
    if (!rc) {
      plan->generation = gen;
      *slot = plan;
    }
  }
  if (rc == ACM_GPU_E_INELIGIBLE && classes) {
    R->path = ACM_SCAN_PATH_CPU_LOOP;
    return ACM_GPU_OK;
  }
  R->plan = plan;
  return rc;
}
} // namespace

namespace {
/* when a call leaves its route in acm_scan_path.  The calls differ, and each keeps its own rule
 * here: acm_scan and acm_scan_batch record whatever their scan returned, acm_tally and acm_lookup only a scan that
 * succeeded, acm_select, acm_scan_words, acm_scan_chars, acm_scan_anchored and acm_scan_from also one that found more records than there was room for,
 * acm_replace, acm_tokenize, acm_grep, acm_grep_lines, acm_tally_batch, acm_rules, acm_score, acm_index, acm_scan_patterns, acm_scan_chains, acm_scan_approx and
 * acm_scan_edit also one whose output had no room, acm_context either of the two. */
enum class RecordPath { Always, OnSuccess, OnSuccessOrOverflow };

/* what every machine-level call does around its scan: the route, the machine's plan lock, the
 * cached plan (GPU paths), then host_loop (declared symbol size) or on_gpu (plan), the path for
 * acm_scan_path, the unlock */
template <typename HostLoop, typename OnGpu>
int
routed_scan (ACMachine *machine, RecordPath record, HostLoop host_loop, OnGpu on_gpu) {
  ScanRoute R;
  int rc = scan_route (machine, &R);
  if (rc)
    return rc;
  acm_internal_plan_lock (machine);
  if (R.path != ACM_SCAN_PATH_CPU_LOOP)
    rc = route_plan (machine, &R);
  if (!rc) {
    rc = R.path == ACM_SCAN_PATH_CPU_LOOP ? host_loop (R.said) : on_gpu (R.plan);
    if (record == RecordPath::Always || !rc || (record == RecordPath::OnSuccessOrOverflow && rc == ACM_GPU_E_OVERFLOW))
      acm_internal_set_scan_path (machine, R.path);
  }
  acm_internal_plan_unlock (machine);
  return rc;
}
} // namespace

/* The twenty-two calls below run on the same route, the same cached plan, under the same lock. */
extern "C" int
acm_scan (ACMachine *machine, const void *text, uint64_t n_symbols, ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  if (!machine || !n_found)
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::Always, [&] (uint32_t said) { return acm_internal_cpu_scan (machine, text, n_symbols, said, records, capacity, n_found); },
    [&] (ACMPlan *plan) { return acm_gpu_scan_host (plan, text, n_symbols, 0, 0, records, capacity, n_found); });
}

/* the same on a batch of texts (include/acm_gpu.h) */
extern "C" int
acm_scan_batch (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, ACMRecord *records, uint32_t *text_id,
                uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  if (!machine || !n_found || (capacity && !records) || !batch_args_ok (text, offsets, n_texts, 1ull << 32))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::Always,
    [&] (uint32_t said) { return acm_internal_cpu_scan_batch (machine, text, offsets, n_texts, said, records, text_id, first, capacity, n_found); },
    [&] (ACMPlan *plan) { return acm_gpu_scan_batch_host (plan, text, offsets, n_texts, records, text_id, first, capacity, n_found); });
}

/* the per-keyword tally (include/acm_gpu.h) */
extern "C" int
acm_tally (ACMachine *machine, const void *text, uint64_t n_symbols, uint64_t *tally, uint64_t n_keywords, uint64_t *total) {
  if (!machine || !tally || (n_symbols && !text))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccess, [&] (uint32_t said) { return acm_internal_cpu_tally (machine, text, n_symbols, said, tally, n_keywords, total); },
    [&] (ACMPlan *plan) { return acm_gpu_tally_host (plan, text, n_symbols, tally, n_keywords, total); });
}

/* the leftmost-longest selection (include/acm_gpu.h) */
extern "C" int
acm_select (ACMachine *machine, const void *text, uint64_t n_symbols, ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  if (!machine || !n_found || (n_symbols && !text) || (capacity && !records))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) { return acm_internal_cpu_select (machine, text, n_symbols, said, records, capacity, n_found); },
    [&] (ACMPlan *plan) { return acm_gpu_scan_select_host (plan, text, n_symbols, 0, records, capacity, n_found); });
}

/* the minimum-cost tiling (include/acm_segment.h) */
extern "C" int
acm_segment (ACMachine *machine, const void *text, uint64_t n_symbols, const uint32_t *cost, uint64_t n_keywords, uint32_t gap_cost,
             ACMRecord *records, uint64_t capacity, uint64_t *n_found, uint64_t sums[2]) {
  if (!machine || !n_found || (n_symbols && !text) || (capacity && !records) || !segment_args_ok (cost, n_keywords, gap_cost))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) { return acm_internal_cpu_segment (machine, text, n_symbols, said, cost, n_keywords, gap_cost, records, capacity, n_found, sums); },
    [&] (ACMPlan *plan) {
      return acm_gpu_scan_segment_host (plan, text, n_symbols, 0, nullptr, 0, cost, n_keywords, gap_cost, records, capacity, n_found, sums);
    });
}

/* whole-word matches of one text (include/acm_gpu.h) */
extern "C" int
acm_scan_words (ACMachine *machine, const void *text, uint64_t n_symbols, const void *ranges, uint32_t n_ranges, uint32_t flags, ACMRecord *records,
                uint64_t capacity, uint64_t *n_found) {
  if (!machine || !n_found || (n_symbols && !text) || (capacity && !records))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) { return acm_internal_cpu_scan_words (machine, text, n_symbols, said, ranges, n_ranges, flags, records, capacity, n_found); },
    [&] (ACMPlan *plan) { return acm_gpu_scan_words_host (plan, text, n_symbols, 0, nullptr, 0, ranges, n_ranges, flags, records, capacity, n_found); });
}

/* the matches of one byte text with their places in code points or UTF-16 units (include/acm_chars.h) */
extern "C" int
acm_scan_chars (ACMachine *machine, const void *text, uint64_t n_symbols, uint32_t unit, ACMRecord *records, uint64_t *char_start, uint32_t *char_len,
                uint8_t *edge, uint64_t capacity, uint64_t *n_found) {
  if (!machine || !n_found || (n_symbols && !text) || (capacity && !records) || !chars_unit_ok (unit) || (!char_start && !char_len && !edge))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) { return acm_internal_cpu_scan_chars (machine, text, n_symbols, said, unit, records, char_start, char_len, edge, capacity, n_found); },
    [&] (ACMPlan *plan) {
      return acm_gpu_scan_chars_host (plan, text, n_symbols, 0, nullptr, 0, unit, records, char_start, char_len, edge, capacity, n_found);
    });
}

/* the matches of one text with the text around them (include/acm_gpu.h) */
extern "C" int
acm_context (ACMachine *machine, const void *text, uint64_t n_symbols, ACMRecord *records, uint64_t capacity, uint64_t *n_found, uint32_t before,
             uint32_t after, uint32_t flags, void *out, uint64_t out_capacity, uint64_t *out_symbols, uint64_t *n_snippets, uint64_t *snip_lo,
             uint64_t *out_offsets, uint32_t *snip_text, uint32_t *rec_snip, int64_t *rec_at) {
  if (!machine || !n_found || !out_symbols || !n_snippets || capacity >= (1ull << 31) || (n_symbols && !text) || (out_capacity && !out) ||
      !context_flags_ok (flags, nullptr))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_context (machine, text, n_symbols, said, records, capacity, n_found, before, after, flags, out, out_capacity, out_symbols,
                                       n_snippets, snip_lo, out_offsets, snip_text, rec_snip, rec_at);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_scan_context_host (plan, text, n_symbols, 0, nullptr, 0, records, capacity, n_found, before, after, flags, out, out_capacity,
                                        out_symbols, n_snippets, snip_lo, out_offsets, snip_text, rec_snip, rec_at);
    });
}

/* anchored matches and the dictionary lookup of a batch (include/acm_gpu.h) */
extern "C" int
acm_scan_anchored (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t mode, ACMRecord *records,
                   uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  if (!machine || !n_found || !anchored_mode_ok (mode) || (capacity && !records) || !batch_args_ok (text, offsets, n_texts, ANCHORED_MOST_TEXTS))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_scan_anchored (machine, text, offsets, n_texts, said, mode, records, text_id, first, capacity, n_found);
    },
    [&] (ACMPlan *plan) { return acm_gpu_scan_anchored_host (plan, text, offsets, n_texts, mode, records, text_id, first, capacity, n_found); });
}

extern "C" int
acm_lookup (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t *whole_id, uint32_t *prefix_id,
            uint32_t *prefix_len) {
  if (!machine || (!whole_id && !prefix_id && !prefix_len) || !batch_args_ok (text, offsets, n_texts, 1ull << 32))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccess,
    [&] (uint32_t said) { return acm_internal_cpu_lookup (machine, text, offsets, n_texts, said, whole_id, prefix_id, prefix_len); },
    [&] (ACMPlan *plan) { return acm_gpu_lookup_host (plan, text, offsets, n_texts, whole_id, prefix_id, prefix_len); });
}

/* search-and-replace (include/acm_gpu.h) */
extern "C" int
acm_replace (ACMachine *machine, const void *text, uint64_t n_symbols, const void *repl_data, const uint64_t *repl_off, uint64_t n_keywords, void *out,
             uint64_t out_capacity, uint64_t *out_symbols, uint64_t *n_replaced) {
  if (!machine || !out_symbols || (n_symbols && !text) || (out_capacity && !out) || (!repl_off && !repl_data))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_replace (machine, text, n_symbols, said, repl_data, repl_off, n_keywords, out, out_capacity, out_symbols, n_replaced);
    },
    [&] (ACMPlan *plan) { return acm_gpu_scan_replace_host (plan, text, n_symbols, repl_data, repl_off, n_keywords, out, out_capacity, out_symbols, n_replaced); });
}

/* tokenising (include/acm_gpu.h) */
extern "C" int
acm_tokenize (ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const uint32_t *tok_of,
              uint64_t n_keywords, uint32_t gap_base, uint32_t mode, uint32_t *tok_id, uint64_t *tok_start, uint32_t *tok_len, uint64_t token_capacity,
              uint64_t *n_tokens, uint64_t *tok_first, uint64_t *n_selected) {
  if (!machine || !n_tokens || (n_symbols && !text) || (!offsets && tok_first) || mode > ACM_TOKENS_GAP_DROP ||
      !optional_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  if (tok_of && n_keywords < acm_nb_keywords (machine)) /* the table covers every keyword of the machine, on every path */
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_tokenize (machine, text, n_symbols, said, offsets, n_texts, tok_of, n_keywords, gap_base, mode, tok_id, tok_start, tok_len,
                                        token_capacity, n_tokens, tok_first, n_selected);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_scan_tokens_host (plan, text, n_symbols, offsets, n_texts, tok_of, n_keywords, gap_base, mode, tok_id, tok_start, tok_len,
                                       token_capacity, n_tokens, tok_first, n_selected);
    });
}

/* grep over a batch (include/acm_gpu.h) */
extern "C" int
acm_grep (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t flags, uint64_t *hits, uint32_t *kept,
          uint64_t *n_kept, uint64_t *total, void *out, uint64_t out_capacity, uint64_t *out_offsets, uint64_t *out_symbols) {
  if (!machine || !n_kept || flags > ACM_GREP_INVERT || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_grep (machine, text, offsets, n_texts, said, flags, hits, kept, n_kept, total, out, out_capacity, out_offsets, out_symbols);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_grep_host (plan, text, offsets, n_texts, flags, hits, kept, n_kept, total, out, out_capacity, out_offsets, out_symbols);
    });
}

/* grep over a raw buffer, split at delimiters first (include/acm_gpu.h) */
extern "C" int
acm_grep_lines (ACMachine *machine, const void *text, uint64_t n_symbols, const void *delims, uint32_t n_delims, uint32_t split_flags, uint32_t grep_flags,
                uint64_t *n_texts, uint64_t *n_kept, uint64_t *total, void *out, uint64_t out_capacity, uint64_t *out_symbols, uint64_t texts_capacity,
                uint64_t *offsets, uint64_t *hits, uint32_t *kept, uint64_t *out_offsets) {
  if (!machine || !n_texts || !n_kept || !split_args_ok (delims, n_delims, split_flags) || grep_flags > ACM_GREP_INVERT || (n_symbols && !text))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_grep_lines (machine, text, n_symbols, said, delims, n_delims, split_flags, grep_flags, n_texts, n_kept, total, out,
                                          out_capacity, out_symbols, texts_capacity, offsets, hits, kept, out_offsets);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_grep_lines_host (plan, text, n_symbols, delims, n_delims, split_flags, grep_flags, n_texts, n_kept, total, out, out_capacity,
                                      out_symbols, texts_capacity, offsets, hits, kept, out_offsets);
    });
}

/* per-text keyword counts of a batch (include/acm_gpu.h) */
extern "C" int
acm_tally_batch (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, uint64_t *row_ptr, uint32_t *col, uint64_t *val,
                 uint64_t nnz_capacity, uint64_t *nnz, uint64_t *total) {
  if (!machine || !row_ptr || !nnz || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) { return acm_internal_cpu_tally_batch (machine, text, offsets, n_texts, said, row_ptr, col, val, nnz_capacity, nnz, total); },
    [&] (ACMPlan *plan) { return acm_gpu_tally_batch_host (plan, text, offsets, n_texts, row_ptr, col, val, nnz_capacity, nnz, total); });
}

/* keyword rules per text of a batch (include/acm_gpu.h) */
extern "C" int
acm_rules (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, const ACMRuleTerm *terms, const uint64_t *rule_ptr,
           const uint32_t *need, uint64_t n_rules, uint64_t *fired_ptr, uint32_t *fired, uint64_t fired_capacity, uint64_t *n_fired, uint64_t *total) {
  if (!machine || !fired_ptr || !n_fired || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_rules (machine, text, offsets, n_texts, said, terms, rule_ptr, need, n_rules, fired_ptr, fired, fired_capacity, n_fired,
                                     total);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_rules_host (plan, text, offsets, n_texts, terms, rule_ptr, need, n_rules, fired_ptr, fired, fired_capacity, n_fired, total);
    });
}

/* weighted scores per text of a batch (include/acm_score.h) */
extern "C" int
acm_score (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, const ACMScoreTerm *terms, const uint64_t *class_ptr,
           const int64_t *bias, const int64_t *threshold, uint64_t n_classes, uint64_t *kept_ptr, uint32_t *kept_class, int64_t *kept_score,
           uint64_t kept_capacity, uint64_t *n_kept, uint32_t *best, uint32_t k, uint64_t *class_hits, uint32_t *top_n, uint32_t *top_text,
           int64_t *top_score, uint64_t *total) {
  if (!machine || !kept_ptr || !n_kept || k > ACM_SCORE_TOP_MAX || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_score (machine, text, offsets, n_texts, said, terms, class_ptr, bias, threshold, n_classes, kept_ptr, kept_class, kept_score,
                                     kept_capacity, n_kept, best, k, class_hits, top_n, top_text, top_score, total);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_score_host (plan, text, offsets, n_texts, terms, class_ptr, bias, threshold, n_classes, kept_ptr, kept_class, kept_score,
                                 kept_capacity, n_kept, best, k, class_hits, top_n, top_text, top_score, total);
    });
}

/* the inverted index of a batch (include/acm_index.h) */
extern "C" int
acm_index (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, uint64_t text_base, uint64_t *post_ptr, uint64_t n_keywords,
           uint32_t *post_text, uint64_t *post_count, uint64_t post_capacity, uint64_t *nnz, uint64_t *total) {
  if (!machine || !post_ptr || !nnz || n_keywords >= (1ull << 32) || text_base > (1ull << 32) || text_base + n_texts > (1ull << 32) ||
      post_capacity >= (1ull << 31) || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      if (n_keywords < acm_nb_keywords (machine))
        return (int)ACM_GPU_E_ARG;
      /* tally_batch's host loop into a room of the call's own, grown once to what the matrix needs */
      std::vector<uint64_t> row_ptr (n_texts + 1), val;
      std::vector<uint32_t> col;
      uint64_t room = 1024, found = 0;
      int rc = ACM_GPU_OK;
      for (int attempt = 0; attempt < 2; attempt++) {
        col.resize (room);
        val.resize (room);
        rc = acm_internal_cpu_tally_batch (machine, text, offsets, n_texts, said, row_ptr.data (), col.data (), val.data (), room, &found, total);
        if (rc != ACM_GPU_E_OVERFLOW)
          break;
        room = found;
      }
      if (rc == ACM_GPU_E_OVERFLOW) /* (the second room is what the first attempt asked for: never expected) */
        rc = ACM_GPU_E_INTERNAL;
      return rc ? rc
                : acm_index_matrix (row_ptr.data (), col.data (), val.data (), n_texts, n_keywords, text_base, post_ptr, post_text, post_count,
                                    post_capacity, nnz);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_index_host (plan, text, offsets, n_texts, text_base, post_ptr, n_keywords, post_text, post_count, post_capacity, nnz, total);
    });
}

/* the co-occurrence matrix of a batch (include/acm_cooccur.h) */
extern "C" int
acm_cooccur (ACMachine *machine, const void *text, const uint64_t *offsets, uint64_t n_texts, uint64_t n_keywords, uint32_t flags, uint64_t row_limit,
             uint64_t *co_ptr, uint32_t *co_col, uint64_t *co_val, uint64_t out_capacity, uint64_t *nnz, uint64_t *cross, uint64_t *skipped,
             uint64_t *total) {
  if (!machine || !co_ptr || !nnz || n_keywords >= (1ull << 32) || (flags & ~(ACM_COOCCUR_PRODUCT | ACM_COOCCUR_DIAGONAL)) ||
      out_capacity >= (1ull << 31) || !batch_args_ok (text, offsets, n_texts, 1ull << 31))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      if (n_keywords < acm_nb_keywords (machine))
        return (int)ACM_GPU_E_ARG;
      /* tally_batch's host loop into a room of the call's own, grown once to what the matrix needs */
      std::vector<uint64_t> row_ptr (n_texts + 1), val;
      std::vector<uint32_t> col;
      uint64_t room = 1024, found = 0;
      int rc = ACM_GPU_OK;
      for (int attempt = 0; attempt < 2; attempt++) {
        col.resize (room);
        val.resize (room);
        rc = acm_internal_cpu_tally_batch (machine, text, offsets, n_texts, said, row_ptr.data (), col.data (), val.data (), room, &found, total);
        if (rc != ACM_GPU_E_OVERFLOW)
          break;
        room = found;
      }
      if (rc == ACM_GPU_E_OVERFLOW) /* (the second room is what the first attempt asked for: never expected) */
        rc = ACM_GPU_E_INTERNAL;
      return rc ? rc
                : acm_cooccur_matrix (row_ptr.data (), col.data (), val.data (), n_texts, n_keywords, flags, row_limit, co_ptr, co_col, co_val,
                                      out_capacity, nnz, cross, skipped);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_cooccur_host (plan, text, offsets, n_texts, n_keywords, flags, row_limit, co_ptr, co_col, co_val, out_capacity, nnz, cross, skipped,
                                   total);
    });
}

/* keyword patterns with don't-care gaps (include/acm_gpu.h) */
extern "C" int
acm_scan_patterns (ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const ACMPatternTerm *terms,
                   const uint64_t *pat_ptr, uint64_t n_patterns, ACMRecord *out, uint64_t out_capacity, uint64_t *n_found) {
  if (!machine || !n_found || (n_symbols && !text) || (out_capacity && !out) || !optional_offsets_ok (offsets, n_texts, n_symbols) ||
      acm_internal_patterns_machine_check (machine, terms, pat_ptr, n_patterns))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_scan_patterns (machine, text, n_symbols, said, offsets, n_texts, terms, pat_ptr, n_patterns, out, out_capacity, n_found);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_scan_patterns_host (plan, text, n_symbols, 0, offsets, n_texts, terms, pat_ptr, n_patterns, out, out_capacity, n_found);
    });
}

/* keyword chains with bounded gaps (include/acm_gpu.h) */
extern "C" int
acm_scan_chains (ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const ACMChainTerm *terms,
                 const uint64_t *chain_ptr, uint64_t n_chains, ACMRecord *out, uint64_t out_capacity, uint64_t *n_found) {
  if (!machine || !n_found || (n_symbols && !text) || (out_capacity && !out) || !optional_offsets_ok (offsets, n_texts, n_symbols) ||
      acm_internal_chains_machine_check (machine, terms, chain_ptr, n_chains))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_scan_chains (machine, text, n_symbols, said, offsets, n_texts, terms, chain_ptr, n_chains, out, out_capacity, n_found);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_scan_chains_host (plan, text, n_symbols, 0, offsets, n_texts, terms, chain_ptr, n_chains, out, out_capacity, n_found);
    });
}

/* unordered keyword proximity (include/acm_near.h) */
extern "C" int
acm_scan_near (ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const uint32_t *terms,
               const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups, ACMRecord *out, uint64_t out_capacity, uint64_t *n_found) {
  if (!machine || !n_found || (n_symbols && !text) || (out_capacity && !out) || !optional_offsets_ok (offsets, n_texts, n_symbols) ||
      acm_internal_near_machine_check (machine, terms, group_ptr, groups, n_groups))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) {
      return acm_internal_cpu_scan_near (machine, text, n_symbols, said, offsets, n_texts, terms, group_ptr, groups, n_groups, out, out_capacity, n_found);
    },
    [&] (ACMPlan *plan) {
      return acm_gpu_scan_near_host (plan, text, n_symbols, 0, offsets, n_texts, terms, group_ptr, groups, n_groups, out, out_capacity, n_found);
    });
}

/* keywords with up to k mismatches, and within edit distance k (include/acm_gpu.h).  Verification is bitwise on the device, so a
 * machine with another comparator runs the caller loop and the host pass under its comparator, whatever its symbol size. */
namespace {
int
scan_set (Metric metric, ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const void *spell_data,
          const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets,
          const ACMTemplateSpec *tpl, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  if (!machine || !n_found || (n_symbols && !text) || (out_capacity && !out) || !optional_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  const bool edits = metric == Metric::Edits;
  ScanRoute R;
  if (const int rc = scan_route (machine, &R))
    return rc;
  uint32_t sb = R.said;
  if (R.path == ACM_SCAN_PATH_GPU && acm_internal_symbol_bytes (machine, &sb))
    return ACM_GPU_E_INTERNAL;
  if (tpl ? acm_internal_templates_machine_check (machine, sb, tpl)
          : (edits ? acm_internal_edit_machine_check : acm_internal_approx_machine_check) (machine, sb, spell_data, spell_off, k, terms, tgt_ptr, n_targets))
    return ACM_GPU_E_ARG;
  const auto host_loop = [&] (uint32_t said) {
    if (tpl)
      return acm_internal_cpu_scan_templates (machine, text, n_symbols, said, offsets, n_texts, tpl, out, dist, out_capacity, n_found);
    return (edits ? acm_internal_cpu_scan_edit : acm_internal_cpu_scan_approx) (machine, text, n_symbols, said, offsets, n_texts, spell_data, spell_off, k,
                                                                                terms, tgt_ptr, n_targets, out, dist, out_capacity, n_found);
  };
  if (R.path != ACM_SCAN_PATH_GPU) { /* (no class plan is made: the route is the loop itself) */
    acm_internal_plan_lock (machine);
    const int rc = host_loop (R.said);
    if (!rc || rc == ACM_GPU_E_OVERFLOW)
      acm_internal_set_scan_path (machine, ACM_SCAN_PATH_CPU_LOOP);
    acm_internal_plan_unlock (machine);
    return rc;
  }
  return routed_scan (machine, RecordPath::OnSuccessOrOverflow, host_loop, [&] (ACMPlan *plan) {
    return scan_set_host (metric, ScanJoinHost{ plan, text, n_symbols, 0, offsets, n_texts, out, dist, out_capacity, n_found }, spell_data, spell_off, k, terms,
                          tgt_ptr, n_targets, tpl);
  });
}
} // namespace

extern "C" int
acm_scan_approx (ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const void *spell_data,
                 const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets, ACMRecord *out,
                 uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  return scan_set (Metric::Mismatches, machine, text, n_symbols, offsets, n_texts, spell_data, spell_off, k, terms, tgt_ptr, n_targets, nullptr, out, dist,
                   out_capacity, n_found);
}

extern "C" int
acm_scan_edit (ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const void *spell_data,
               const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets, ACMRecord *out,
               uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  return scan_set (Metric::Edits, machine, text, n_symbols, offsets, n_texts, spell_data, spell_off, k, terms, tgt_ptr, n_targets, nullptr, out, dist,
                   out_capacity, n_found);
}

extern "C" int
acm_scan_templates (ACMachine *machine, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, const ACMTemplateSpec *spec,
                    ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  if (!spec)
    return ACM_GPU_E_ARG;
  return scan_set (Metric::Templates, machine, text, n_symbols, offsets, n_texts, spec->spell_data, spec->spell_off, spec->k, spec->terms, spec->tgt_ptr,
                   spec->n_templates, spec, out, dist, out_capacity, n_found);
}

/* acm_scan continued from a cursor (include/acm_gpu.h): the reference's own `const ACState *`, in
 * and out.  GPU paths: the cursor's spelling (its parent links, as acm_get_match walks them) goes
 * in front of the text with the emit boundary behind it; the cursor afterwards is a walk with the
 * product's own acm_match from the root over the last lmax symbols of spelling + text (lmax, not
 * lmax - 1: the cursor may sit on a state of full depth). */
extern "C" int
acm_scan_from (ACMachine *machine, const ACState **cursor, const void *text, uint64_t n_symbols, ACMRecord *records, uint64_t capacity,
               uint64_t *n_found) {
  if (!machine || !cursor || !*cursor || (*cursor)->machine != machine || !n_found || (n_symbols && !text) || (capacity && !records))
    return ACM_GPU_E_ARG;
  return routed_scan (
    machine, RecordPath::OnSuccessOrOverflow,
    [&] (uint32_t said) { return acm_internal_cpu_scan_from (machine, cursor, text, n_symbols, said, records, capacity, n_found); },
    [&] (ACMPlan *plan) {
      const uint32_t sb = plan->text_sym_bytes;
      const uint64_t depth = (*cursor)->depth;
      std::vector<unsigned char> spelling ((size_t)depth * sb);
      uint64_t k = depth;
      for (const ACState *s = *cursor; s->parent; s = s->parent)
        memcpy (spelling.data () + (size_t)--k * sb, s->letter, sb);
      const int rc = scan_host_prefixed (plan, spelling.data (), depth, text, n_symbols, depth, 0, records, capacity, n_found);
      if (rc)
        return rc;
      for (uint64_t r = 0; r < *n_found; r++)
        records[r].end_pos -= depth;
      const uint64_t all = depth + n_symbols, lmax = plan_lmax (plan);
      const ACState *s = acm_internal_root (machine);
      for (uint64_t i = all > lmax ? all - lmax : 0; i < all; i++)
        (void)acm_match (&s, i < depth ? spelling.data () + (size_t)i * sb : static_cast<const unsigned char *> (text) + (size_t)(i - depth) * sb);
      *cursor = s;
      return rc;
    });
}

#ifdef ACM_DIAG
extern "C" int
acm_gpu_diag_read (unsigned long long *out, unsigned waves) {
  HIP_TRY (hipMemcpyFromSymbol (out, HIP_SYMBOL (g_acm_diag), sizeof (unsigned long long) * 8 * (waves < 8192 ? waves : 8192)));
  return ACM_GPU_OK;
}
#endif

/* ------------------------------------------------------------------ synthetic workload */
extern "C" int
acm_gpu_synth_text (int device, void *d_text, uint64_t n, uint64_t global_begin, uint32_t sym_bytes, uint32_t vocab,
                    const void *d_kw_data, const uint32_t *d_kw_off, uint32_t n_kw, void *stream) {
  if (!d_text || (global_begin & 4095) || (sym_bytes != 1 && sym_bytes != 4) || (sym_bytes == 4 && !vocab))
    return ACM_GPU_E_ARG;
  HIP_TRY (hipSetDevice (device));
  hipStream_t st = static_cast<hipStream_t> (stream);
  if (n == 0)
    return ACM_GPU_OK;
  dim3 g (4096), b (256);
  if (sym_bytes == 1)
    hipLaunchKernelGGL (synth_text_kernel<uint8_t>, g, b, 0, st, static_cast<uint8_t *> (d_text), n, global_begin, vocab,
                        static_cast<const uint8_t *> (d_kw_data), d_kw_off, n_kw);
  else
    hipLaunchKernelGGL (synth_text_kernel<uint32_t>, g, b, 0, st, static_cast<uint32_t *> (d_text), n, global_begin, vocab,
                        static_cast<const uint32_t *> (d_kw_data), d_kw_off, n_kw);
  HIP_TRY (hipGetLastError ());
  return ACM_GPU_OK;
}
