/* dev_tally_batch.h -- per-text keyword counts of a batch: C[t][k] = how often keyword k occurs in
 * text t, as a CSR matrix (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * C is a histogram of the (text, keyword) PAIRS of a batch's records, as the tally is one of their
 * keywords and grep's hits one of their texts: the record scan of any plan kind (no scan kernel
 * touched), window by window into a record area of `capacity` records in the caller's scratch, and
 * a reduction of what every window found to distinct pairs.  The passes, all on the caller's stream:
 *   1. batch_index_kernel<false> (dev_batch.h), once, in front of the windows: grep's pass 1.
 *   2. tb_pairs_kernel, behind every window's scan: grep's protocol on `need`, then a grid-stride
 *      loop over the records, one 16-byte load per lane; the record's text and whether it counts by
 *      grep_record_text (dev_grep.h: the one helper of both); key = text << 32 | keyword_id.  A
 *      block combines its keys in an open-addressing hash table in LDS: a slot is a 64-bit key and
 *      a 32-bit count, claimed with a 64-bit LDS compare-and-swap; the empty slot is all ones (no
 *      key: text ids are below 2^31).  One keyword hitting all through one text would put a whole
 *      wave on one slot: the lanes that hold the key of the wave's first kept lane add ONCE (two
 *      ballots, a popcount, one insert by one lane), as grep_hits_kernel does for its hot text.
 *      An insert looks at TB_PROBES slots at the most and then FAILS; a block whose round had a
 *      failed insert flushes its table and the failed lanes try again.  This is the load limit of
 *      the table: a probe sequence that long means a crowded table, and it needs no count of used
 *      slots read by every lane between two barriers -- one barrier per round of 256 records.
 *      (A table smaller than a round's distinct keys -- ACM_GPU_TALLY_BATCH_SLOTS=8 -- flushes
 *      several times per round.)  A flush, also at the block's end: one atomic per block reserves
 *      room in the scratch area of PARTIAL pairs, then (key, count) per used slot; beyond
 *      pair_capacity it counts but does not write.  The kept records are counted too: that count is
 *      `total` and, when the partial pairs overflowed, *d_need_pairs -- every partial pair stands
 *      for one kept record or more, so the kept-record count always suffices, and unlike the number
 *      of partial pairs it does not depend on the order in which the scan left its records.
 *      A keyword_id that is no keyword of the plan raises the plan's error flag and is not counted.
 *      Table: 4,096 slots of 12 bytes = 48 KiB (below the 64 KiB a block gets without asking; two
 *      blocks fit the 160 KiB of a CU, and the grid is two blocks per CU: dev_tally.h's reasoning).
 *   3. Once, behind the last window: tb_hist_kernel counts the partial pairs per text, an exclusive
 *      sum over n_texts + 1 (hipCUB) gives every text's bucket, tb_scatter_kernel moves the pairs
 *      there (the histogram counted down is the cursor) as (keyword, 64-bit count, text).
 *   4. tb_merge_kernel: a block takes 256 consecutive texts; their buckets are one consecutive run.
 *      When the run has at most R entries the block sorts it in LDS by (text, keyword) -- a bitonic
 *      network over the next power of two, padded with all ones --, finds the first entry of every
 *      distinct key, ranks those by ballot, adds up each key's run and writes the merged rows to
 *      the front of their buckets (in a second area: the partial pairs' own, which is free by now)
 *      and their lengths to row_nnz[].  A run with more entries is tried in 16 groups of 16 texts,
 *      then text by text; a single text with more than R entries goes on the list of WIDE rows.
 *      tb_wide_kernel, TB_WIDE_BLOCKS blocks, takes the wide rows one per block: adds the row into
 *      the block's own histogram of n_keywords 64-bit counters in scratch, sweeps it in keyword
 *      order with ballot ranks and zeroes it again -- slow and correct, so that no input is refused
 *      (ACM_GPU_SELECT_FORM_WALK's role).  A block zeroes its histogram only when a wide row exists.
 *      R = 2,048 (40 KiB of LDS); ACM_GPU_TALLY_BATCH_ROW=<entries> sets another (tests).  There is
 *      no per-plan choice of form, so none is reported.
 *   5. An exclusive sum of row_nnz[] (hipCUB) into scratch; tb_finish_kernel copies the row
 *      pointers and the rows to the caller's arrays (every bucket entry knows its text: a flat
 *      grid-stride loop) and one lane writes the scalars by the overflow rules.  The row pointers go
 *      through scratch so that a call with bad offsets writes none of the caller's arrays.
 * Every pass behind the windows returns at once when the call has stopped (bad offsets, a window
 * over `capacity`, partial pairs over `pair_capacity`).
 * Launch geometry never depends on the number of records, pairs or texts: capped grids, grid-stride
 * loops.  Nothing reads a count back to the host. */
constexpr uint32_t TB_THREADS = 256, TB_WAVES = TB_THREADS / WAVE;
constexpr uint32_t TB_SLOTS_DEFAULT = 4096, TB_SLOTS_MIN = 8, TB_SLOTS_MAX = 4096;
constexpr uint32_t TB_PROBES = 16;
constexpr uint32_t TB_ROW_DEFAULT = 2048, TB_ROW_MAX = 2048;
constexpr uint32_t TB_TILE = TB_THREADS, TB_SUBTILE = 16; /* texts per group of pass 4 */
constexpr uint32_t TB_WIDE_BLOCKS = 8;
constexpr unsigned long long TB_EMPTY = ~0ull;
static_assert (TB_SLOTS_MAX * 12 <= 64 * 1024 && 2 * TB_SLOTS_MAX * 12 <= 160 * 1024, "two blocks of the pairs kernel share one CU");
static_assert (TB_ROW_MAX * 16 + (TB_ROW_MAX + 1) * 4 <= 64 * 1024 && (TB_ROW_MAX & (TB_ROW_MAX - 1)) == 0, "the merge sorts in LDS");

/* control words at the head of the passes' scratch, cleared in front of every call */
struct TbCtl {
  BatchCtl batch;             /* .bad: offsets[] break the contract (batch_index_kernel) */
  unsigned long long need;    /* largest record count of a window so far */
  unsigned long long kept;    /* records counted so far */
  unsigned long long partial; /* partial pairs reserved so far, also beyond pair_capacity */
  unsigned long long n_wide;  /* rows on the wide list */
};

struct TbK {
  /* pass 2 */
  const ACMRecord *rec;            /* the window's records, in no order */
  uint64_t capacity;               /* of `rec` */
  const unsigned long long *n_dev; /* the window's record count (device) */
  uint64_t read_begin;             /* the window's positions are relative to this symbol of the buffer */
  const uint64_t *offsets;         /* [n_texts + 1] */
  uint64_t n_texts, n_symbols;
  const uint32_t *index;           /* [n_blocks]: text of position b << BATCH_BLOCK_LOG2 */
  uint32_t n_keywords;             /* keywords the plan and its delta report */
  uint32_t slots, shift;           /* of the LDS table (a power of two); 64 - log2 (slots) */
  uint64_t pair_capacity;          /* of every pair area and of d_col, d_val */
  unsigned long long *pkey;        /* [pair_capacity] partial pairs: text << 32 | keyword */
  uint32_t *pcnt;                  /* [pair_capacity] their counts */
  /* pass 3 */
  uint32_t *hist;                  /* [n_texts + 1] partial pairs per text, counted down by the scatter */
  const uint32_t *begin;           /* [n_texts + 1] exclusive sum: the texts' buckets */
  uint32_t *bkw, *btext;           /* [pair_capacity] the bucketed pairs */
  unsigned long long *bval;
  /* pass 4 */
  uint32_t row, row_p2;            /* R and the LDS room in entries, a power of two >= R */
  uint32_t *mcol;                  /* [pair_capacity] merged rows at the front of their buckets (pcnt's memory) */
  unsigned long long *mval;        /* (pkey's memory) */
  unsigned long long *row_nnz;     /* [n_texts + 1], the last entry stays 0 */
  uint32_t *wide;                  /* rows of more than R entries */
  unsigned long long *whist;       /* [TB_WIDE_BLOCKS][n_keywords] */
  /* pass 5 */
  const unsigned long long *row_ptr; /* [n_texts + 1] exclusive sum of row_nnz */
  unsigned long long *d_row_ptr, *d_val, *d_nnz, *d_total, *d_need, *d_need_pairs;
  uint32_t *d_col;
  TbCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* the call reports nothing: bad offsets, a window with more records than there is room for, or
 * more partial pairs than there is room for */
__device__ __forceinline__ bool
tb_stopped (const TbK &K) {
  return K.ctl->batch.bad != 0 || K.ctl->need > K.capacity || K.ctl->partial > K.pair_capacity;
}

/* `add` more of `key` into the block's table; false when TB_PROBES slots hold other keys */
__device__ __forceinline__ bool
tb_insert (unsigned long long *keys, uint32_t *cnts, const TbK &K, unsigned long long key, uint32_t add, uint32_t *used) {
  const uint32_t mask = K.slots - 1, probes = K.slots < TB_PROBES ? K.slots : TB_PROBES;
  const uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> K.shift);
  for (uint32_t p = 0; p < probes; p++) {
    const uint32_t s = (h + p) & mask;
    unsigned long long was = *reinterpret_cast<volatile unsigned long long *> (&keys[s]);
    if (was == TB_EMPTY) {
      was = atomicCAS (&keys[s], TB_EMPTY, key);
      if (was == TB_EMPTY) {
        atomicAdd (used, 1u);
        was = key;
      }
    }
    if (was == key) {
      atomicAdd (&cnts[s], add);
      return true;
    }
  }
  return false;
}

/* the block's table to the partial pairs, and empty again; called by the whole block behind a barrier */
__device__ __forceinline__ void
tb_flush (const TbK &K, unsigned long long *keys, uint32_t *cnts, uint32_t *used, uint32_t *out, unsigned long long *base) {
  if (threadIdx.x == 0) {
    const uint32_t u = *used;
    *base = u ? atomicAdd (&K.ctl->partial, (unsigned long long)u) : 0ull;
    *used = 0;
    *out = 0;
  }
  __syncthreads ();
  const unsigned long long b = *base;
  for (uint32_t s = threadIdx.x; s < K.slots; s += TB_THREADS) {
    const unsigned long long key = keys[s];
    if (key == TB_EMPTY)
      continue;
    const unsigned long long at = b + atomicAdd (out, 1u);
    if (at < K.pair_capacity) {
      K.pkey[at] = key;
      K.pcnt[at] = cnts[s];
    }
    keys[s] = TB_EMPTY;
    cnts[s] = 0;
  }
  __syncthreads ();
}

/* pass 2 */
__global__ __launch_bounds__ (TB_THREADS) void
tb_pairs_kernel (TbK K) {
  extern __shared__ unsigned long long tb_lds[]; /* [slots] keys, [slots] 32-bit counts */
  __shared__ uint32_t s_used, s_out;
  __shared__ unsigned long long s_base;
  const unsigned long long n = *K.n_dev;
  /* an earlier window of this call overflowed: the call reports nothing, only `need` still grows
   * (the value read is that of the earlier kernels; this kernel's own count is checked by itself) */
  const bool lost = K.ctl->need > K.capacity;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicMax (&K.ctl->need, n);
  if (n > K.capacity || lost || K.ctl->batch.bad) /* (uniform in the grid) */
    return;
  unsigned long long *keys = tb_lds;
  uint32_t *cnts = reinterpret_cast<uint32_t *> (tb_lds + K.slots);
  for (uint32_t s = threadIdx.x; s < K.slots; s += TB_THREADS) {
    keys[s] = TB_EMPTY;
    cnts[s] = 0;
  }
  if (threadIdx.x == 0)
    s_used = 0;
  __syncthreads ();
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t stride = (uint64_t)gridDim.x * TB_THREADS;
  unsigned long long kept = 0;
  bool wrong = false;
  /* (the loop's condition is uniform in the block: the barriers see every lane) */
  for (uint64_t base = (uint64_t)blockIdx.x * TB_THREADS; base < n; base += stride) {
    const uint64_t i = base + threadIdx.x;
    bool keep = false;
    uint32_t t = 0, k = 0;
    if (i < n) {
      const uint4 r = *reinterpret_cast<const uint4 *> (&K.rec[i]);
      keep = grep_record_text (r, K.read_begin, K.offsets, K.n_texts, K.n_symbols, K.index, t, wrong);
      k = r.w; /* keyword_id */
      if (keep && k >= K.n_keywords) { /* no keyword of this plan (never expected): reported, not counted */
        wrong = true;
        keep = false;
      }
    }
    const unsigned long long key = ((unsigned long long)t << 32) | k;
    uint32_t add = 0;
    const unsigned long long m = __ballot (keep);
    if (m != 0) {
      const int first = __ffsll (m) - 1;
      const unsigned long long key0 =
        ((unsigned long long)(uint32_t)__shfl ((int)t, first, WAVE) << 32) | (uint32_t)__shfl ((int)k, first, WAVE);
      const unsigned long long same = __ballot (keep && key == key0);
      if (keep) {
        kept++;
        if (key != key0)
          add = 1;
        else if ((int)lane == __ffsll (same) - 1)
          add = (uint32_t)__popcll (same);
      }
    }
    bool pending = add != 0;
    for (;;) {
      if (pending)
        pending = !tb_insert (keys, cnts, K, key, add, &s_used);
      if (!__syncthreads_or (pending))
        break;
      tb_flush (K, keys, cnts, &s_used, &s_out, &s_base);
    }
  }
  tb_flush (K, keys, cnts, &s_used, &s_out, &s_base);
  /* one add per wave into the call's kept records */
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1)
    kept += ((unsigned long long)__shfl_xor ((uint32_t)(kept >> 32), d, WAVE) << 32) | __shfl_xor ((uint32_t)kept, d, WAVE);
  if (lane == 0 && kept)
    atomicAdd (&K.ctl->kept, kept);
  if (wrong && K.error)
    *K.error = 1;
}

/* pass 3 */
__global__ __launch_bounds__ (TB_THREADS) void
tb_hist_kernel (TbK K) {
  if (tb_stopped (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, np = K.ctl->partial;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < np; e += stride)
    atomicAdd (&K.hist[K.pkey[e] >> 32], 1u);
}

__global__ __launch_bounds__ (TB_THREADS) void
tb_scatter_kernel (TbK K) {
  if (tb_stopped (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, np = K.ctl->partial;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < np; e += stride) {
    const unsigned long long key = K.pkey[e];
    const uint32_t t = (uint32_t)(key >> 32);
    const uint64_t at = (uint64_t)K.begin[t] + (atomicSub (&K.hist[t], 1u) - 1u); /* (the histogram counted this pair) */
    if (at < np) {
      K.bkw[at] = (uint32_t)key;
      K.bval[at] = K.pcnt[e];
      K.btext[at] = t;
    }
  }
}

/* pass 4: the rows of texts [ta, tb), whose buckets hold n <= K.row entries from b0 on, merged */
__device__ __forceinline__ void
tb_merge_group (const TbK &K, unsigned long long *skey, unsigned long long *sval, uint32_t *hrank, uint32_t *wave_heads, uint64_t ta, uint64_t tb,
                uint32_t b0, uint32_t n) {
  if (n == 0) /* (row_nnz[] was cleared) */
    return;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  uint32_t p2 = 1;
  while (p2 < n)
    p2 <<= 1;
  for (uint32_t i = threadIdx.x; i < p2; i += TB_THREADS) {
    const bool in = i < n;
    skey[i] = in ? ((unsigned long long)(K.btext[b0 + i] - (uint32_t)ta) << 32) | K.bkw[b0 + i] : TB_EMPTY;
    sval[i] = in ? K.bval[b0 + i] : 0ull;
  }
  __syncthreads ();
  for (uint32_t k = 2; k <= p2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < p2; i += TB_THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const unsigned long long a = skey[i], b = skey[l];
          if ((a > b) == ((i & k) == 0)) {
            const unsigned long long va = sval[i], vb = sval[l];
            skey[i] = b;
            skey[l] = a;
            sval[i] = vb;
            sval[l] = va;
          }
        }
      }
      __syncthreads ();
    }
  /* hrank[i] = distinct keys in front of entry i; hrank[n] = all */
  uint32_t running = 0;
  for (uint32_t c0 = 0; c0 < n; c0 += TB_THREADS) { /* (uniform in the block) */
    const uint32_t i = c0 + threadIdx.x;
    const bool head = i < n && (i == 0 || skey[i] != skey[i - 1]);
    const unsigned long long m = __ballot (head);
    if (lane == 0)
      wave_heads[wave] = (uint32_t)__popcll (m);
    __syncthreads ();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < (int)TB_WAVES; w++) {
      before += w < (int)wave ? wave_heads[w] : 0u;
      all += wave_heads[w];
    }
    if (i < n)
      hrank[i] = running + before + rank_below (m);
    running += all;
    __syncthreads ();
  }
  if (threadIdx.x == 0)
    hrank[n] = running;
  __syncthreads ();
  for (uint32_t i = threadIdx.x; i < n; i += TB_THREADS) {
    const unsigned long long key = skey[i];
    if (i != 0 && key == skey[i - 1])
      continue;
    unsigned long long sum = sval[i];
    for (uint32_t j = i + 1; j < n && skey[j] == key; j++)
      sum += sval[j];
    const uint64_t t = ta + (key >> 32);
    const uint32_t bt = K.begin[t];
    const uint32_t at = bt + (hrank[i] - hrank[bt - b0]); /* (a row's first entry is the first of its key) */
    K.mcol[at] = (uint32_t)key;
    K.mval[at] = sum;
  }
  for (uint64_t t = ta + threadIdx.x; t < tb; t += TB_THREADS)
    K.row_nnz[t] = hrank[K.begin[t + 1] - b0] - hrank[K.begin[t] - b0];
  __syncthreads (); /* (the next group sorts in the same words) */
}

__global__ __launch_bounds__ (TB_THREADS) void
tb_merge_kernel (TbK K) {
  extern __shared__ unsigned long long tb_lds[]; /* [row_p2] keys, [row_p2] values, [row_p2 + 1] 32-bit ranks */
  __shared__ uint32_t wave_heads[TB_WAVES];
  if (tb_stopped (K))
    return;
  unsigned long long *skey = tb_lds, *sval = tb_lds + K.row_p2;
  uint32_t *hrank = reinterpret_cast<uint32_t *> (tb_lds + 2 * (size_t)K.row_p2);
  const uint64_t n_tiles = (K.n_texts + TB_TILE - 1) / TB_TILE;
  /* (every condition below is uniform in the block: the groups' barriers see every lane) */
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t ta = tile * TB_TILE, tb = ta + TB_TILE < K.n_texts ? ta + TB_TILE : K.n_texts;
    if (K.begin[tb] - K.begin[ta] <= K.row) {
      tb_merge_group (K, skey, sval, hrank, wave_heads, ta, tb, K.begin[ta], K.begin[tb] - K.begin[ta]);
      continue;
    }
    for (uint64_t sa = ta; sa < tb; sa += TB_SUBTILE) {
      const uint64_t se = sa + TB_SUBTILE < tb ? sa + TB_SUBTILE : tb;
      if (K.begin[se] - K.begin[sa] <= K.row) {
        tb_merge_group (K, skey, sval, hrank, wave_heads, sa, se, K.begin[sa], K.begin[se] - K.begin[sa]);
        continue;
      }
      for (uint64_t t = sa; t < se; t++) {
        const uint32_t len = K.begin[t + 1] - K.begin[t];
        if (len <= K.row)
          tb_merge_group (K, skey, sval, hrank, wave_heads, t, t + 1, K.begin[t], len);
        else if (threadIdx.x == 0)
          K.wide[atomicAdd (&K.ctl->n_wide, 1ull)] = (uint32_t)t;
      }
    }
  }
}

__global__ __launch_bounds__ (TB_THREADS) void
tb_wide_kernel (TbK K) {
  __shared__ uint32_t wave_some[TB_WAVES];
  if (tb_stopped (K))
    return;
  const uint64_t n_wide = K.ctl->n_wide;
  if (blockIdx.x >= n_wide) /* (uniform in the block) */
    return;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  /* counters that other lanes add to with atomics are read and written past the CU's own cache */
  unsigned long long *hist = K.whist + (size_t)blockIdx.x * K.n_keywords;
  for (uint32_t k = threadIdx.x; k < K.n_keywords; k += TB_THREADS)
    __hip_atomic_store (&hist[k], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence ();
  __syncthreads ();
  for (uint64_t w = blockIdx.x; w < n_wide; w += gridDim.x) {
    const uint32_t t = K.wide[w], b = K.begin[t], e = K.begin[t + 1];
    for (uint32_t i = b + threadIdx.x; i < e; i += TB_THREADS)
      atomicAdd (&hist[K.bkw[i]], K.bval[i]); /* (bkw[] < n_keywords: the pairs kernel's check) */
    __threadfence ();
    __syncthreads ();
    uint32_t running = 0;
    for (uint32_t k0 = 0; k0 < K.n_keywords; k0 += TB_THREADS) { /* (uniform in the block) */
      const uint32_t k = k0 + threadIdx.x;
      unsigned long long c = 0;
      if (k < K.n_keywords) {
        c = __hip_atomic_load (&hist[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c)
          __hip_atomic_store (&hist[k], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const unsigned long long m = __ballot (c != 0);
      if (lane == 0)
        wave_some[wave] = (uint32_t)__popcll (m);
      __syncthreads ();
      uint32_t before = 0, all = 0;
#pragma unroll
      for (int v = 0; v < (int)TB_WAVES; v++) {
        before += v < (int)wave ? wave_some[v] : 0u;
        all += wave_some[v];
      }
      if (c) { /* (distinct keywords of a row are no more than its entries) */
        const uint32_t at = b + running + before + rank_below (m);
        K.mcol[at] = k;
        K.mval[at] = c;
      }
      running += all;
      __syncthreads ();
    }
    if (threadIdx.x == 0)
      K.row_nnz[t] = running;
    __threadfence ();
    __syncthreads ();
  }
}

/* pass 5 */
__global__ __launch_bounds__ (TB_THREADS) void
tb_finish_kernel (TbK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool stop = tb_stopped (K);
  if (me == 0) {
    const bool no_pairs = K.ctl->batch.bad != 0 || K.ctl->need > K.capacity;
    *K.d_need = K.ctl->need;
    *K.d_need_pairs = no_pairs ? 0ull : K.ctl->partial > K.pair_capacity ? K.ctl->kept : K.ctl->partial;
    *K.d_nnz = stop ? 0ull : K.row_ptr[K.n_texts];
    *K.d_total = stop ? 0ull : K.ctl->kept;
  }
  if (stop) /* every other output stays as it was */
    return;
  for (uint64_t t = me; t <= K.n_texts; t += stride)
    K.d_row_ptr[t] = K.row_ptr[t];
  const uint64_t np = K.ctl->partial;
  for (uint64_t e = me; e < np; e += stride) {
    const uint32_t t = K.btext[e];
    const uint64_t j = e - K.begin[t];
    if (j < K.row_nnz[t]) {
      const uint64_t at = K.row_ptr[t] + j; /* (below nnz <= partial pairs <= pair_capacity) */
      K.d_col[at] = K.mcol[e];
      K.d_val[at] = K.mval[e];
    }
  }
}
