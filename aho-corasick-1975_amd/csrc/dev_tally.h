/* dev_tally.h -- per-keyword match counts: how often every keyword of the dictionary occurs.
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The tally of a text is a histogram of the keyword_id field of its RECORDS, so it is the record
 * scan of any plan kind (no scan kernel touched) and one pass over what that scan found.  The text
 * is scanned window by window into a record area of `capacity` records in the caller's scratch
 * (records need no order: no order pass runs); behind every window's scan, on its stream:
 *   tally_records_kernel: reads the window's record count on the device (as dev_order.h and
 *      dev_batch.h do), a grid-stride loop over the records, one 16-byte load and one add per lane,
 *      into `hist`, a SCRATCH histogram of 64-bit counters -- not the caller's.  Two forms:
 *        LDS    (at most TALLY_LDS_KEYWORDS keywords): a block keeps 32-bit counters in LDS (it sees
 *               fewer than 2^31 records), adds with no-return LDS atomics and hands every non-zero
 *               counter to `hist` with one 64-bit global atomic at its end;
 *        global (more keywords, or ACM_GPU_TALLY=global): no-return 64-bit global atomics straight
 *               into `hist`.
 *      TALLY_LDS_KEYWORDS = 16,384: its counters are 64 KiB, the most a block gets without asking
 *      for more than the default limit, and two such blocks (128 KiB) fit the 160 KiB of one CU, so
 *      that one block's loads overlap the other's zeroing and hand-over.  A block takes LDS for the
 *      dictionary's keywords only (dynamic LDS), not for the threshold.
 *      A keyword_id that is no keyword of the plan raises the plan's error flag and is never used
 *      as an index.  A window whose count exceeds `capacity` is not tallied at all; every window's
 *      count goes into TallyCtl::need by atomicMax, so that the word ends up as the largest window
 *      count of the call -- greater than `capacity` iff some window overflowed.
 *   tally_finish_kernel, once, behind the last window: without overflow d_tally[k] += hist[k] and
 *      *d_total += hist[k] (zeroed in front of it); with overflow neither is touched.  *d_need =
 *      TallyCtl::need either way.  The scratch histogram is there for this: the caller's counters
 *      accumulate over calls, an overflowing call must not leave half a text in them.
 * Launch geometry never depends on the number of records: capped grids, grid-stride loops. */
constexpr uint32_t TALLY_THREADS = 256;
constexpr uint32_t TALLY_LDS_KEYWORDS = 16384;
static_assert (TALLY_LDS_KEYWORDS * sizeof (uint32_t) <= 64 * 1024 && 2 * TALLY_LDS_KEYWORDS * sizeof (uint32_t) <= 160 * 1024,
               "two blocks of the LDS form share one CU");

/* control words at the head of the tally's scratch, cleared in front of every call */
struct TallyCtl {
  unsigned long long need; /* largest record count of a window so far */
  unsigned long long pad;
};

struct TallyK {
  const ACMRecord *rec;            /* the window's records, in no order */
  uint64_t capacity;               /* of `rec` */
  const unsigned long long *n_dev; /* the window's record count (device) */
  unsigned long long *hist;        /* [n_keywords] scratch histogram */
  uint32_t n_keywords;             /* keywords the plan and its delta report */
  TallyCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
  /* tally_finish_kernel */
  unsigned long long *d_tally, *d_total, *d_need;
};

template <bool LDS>
__global__ __launch_bounds__ (TALLY_THREADS) void
tally_records_kernel (TallyK K) {
  extern __shared__ uint32_t tally_lds[]; /* LDS form: [n_keywords] */
  const unsigned long long n = *K.n_dev;
  /* an earlier window of this call overflowed: the call reports nothing, only `need` still grows
   * (the value read is that of the earlier kernels; this kernel's own count is checked by itself) */
  const bool lost = K.ctl->need > K.capacity;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicMax (&K.ctl->need, n);
  if (n > K.capacity || lost) /* (uniform in the grid) */
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < K.n_keywords; k += blockDim.x)
      tally_lds[k] = 0;
    __syncthreads ();
  }
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint4 r = *reinterpret_cast<const uint4 *> (&K.rec[i]);
    const uint32_t k = r.w; /* keyword_id */
    if (k >= K.n_keywords)
      bad = true; /* no keyword of this plan (never expected): reported, not counted */
    else if (LDS)
      atomicAdd (&tally_lds[k], 1u);
    else
      atomicAdd (&K.hist[k], 1ull);
  }
  if (bad && K.error)
    *K.error = 1;
  if (LDS) {
    __syncthreads ();
    for (uint32_t k = threadIdx.x; k < K.n_keywords; k += blockDim.x) {
      const uint32_t c = tally_lds[k];
      if (c)
        atomicAdd (&K.hist[k], (unsigned long long)c);
    }
  }
}

__global__ __launch_bounds__ (TALLY_THREADS) void
tally_finish_kernel (TallyK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long need = K.ctl->need;
  if (me == 0)
    *K.d_need = need;
  if (need > K.capacity) /* all or nothing: the caller's counters stay as they were, *d_total stays 0 */
    return;
  unsigned long long sum = 0;
  for (uint64_t k = me; k < K.n_keywords; k += stride) {
    const unsigned long long c = K.hist[k];
    if (c)
      K.d_tally[k] += c;
    sum += c;
  }
  /* one add per wave into the caller's total */
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1)
    sum += ((unsigned long long)__shfl_xor ((uint32_t)(sum >> 32), d, WAVE) << 32) | __shfl_xor ((uint32_t)sum, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0 && sum)
    atomicAdd (K.d_total, sum);
}
