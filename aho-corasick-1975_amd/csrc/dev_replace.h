/* dev_replace.h -- search-and-replace: REPLACE of a text under a selection (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The input is a selection -- records in canonical order, no two sharing a symbol: what dev_select.h
 * leaves -- its count read on the device, the text and a replacement table (or ONE fill symbol: MASK).
 * The passes, all behind whatever made the selection, on its stream:
 *   a. replace_measure_kernel: every record against the contract (inside the text, behind the record
 *      in front of it, a keyword id of the table) and the table against its own (repl_off never
 *      decreases); delta_j = |R(kw_j)| - length_j, 0 in mask mode, summed per chunk of REPLACE_CHUNK
 *      records, signed 64-bit.  A violation raises the plan's error flag and counts in ctl->n_bad:
 *      every later pass then returns at once, *d_out_symbols = 0.  No address is formed from a record
 *      before this pass has seen it.
 *   b. the exclusive prefix sum over the chunks (hipcub, 64-bit), then replace_starts_kernel: a scan
 *      inside every chunk gives out_start[j] = s_j + the deltas in front of j, to scratch and to the
 *      caller's d_out_start; *d_out_symbols = n_symbols + the sum of all deltas.
 *   c. replace_build_kernel, output-stationary: the output is cut into tiles of whole 16-byte words of
 *      the OUTPUT buffer's own 16-byte grid.  A block finds the last record that begins at or in front
 *      of its tile and the records that begin in front of the tile's end (two 64-way searches of a
 *      wave over out_start[]), stages those records, REPLACE_STAGE at a time, in LDS as segments in
 *      BYTES -- where the replacement begins and ends in the output, where the text goes on behind
 *      the match, where the replacement lies in the table -- and goes on in pieces when the tile
 *      touches more than REPLACE_STAGE.  Every lane makes whole words: a bisection in LDS finds the
 *      segment of the word's first byte; a word that lies wholly inside one stretch of text or one
 *      replacement loads the two aligned 16-byte words of the source that hold it and shifts them
 *      together (whatever (source - destination) mod 16 is); a word that straddles a boundary is put
 *      together byte by byte.  One 16-byte store per word; the first and the last word of the output,
 *      when the buffer does not begin or end on the grid, go by byte stores.  Every output byte is
 *      written once, by one lane; no atomics.  In mask mode the replacement's source is the fill word.
 * The aligned loads of the fast path may take in up to 15 bytes in front of or behind the stretch
 * they copy: bytes of a 16-byte word that holds a byte of the stretch, so of the same page.
 * Launch geometry never depends on the number of records: capped grids, grid-stride loops. */
constexpr uint32_t REPLACE_THREADS = 256, REPLACE_PER = 4, REPLACE_CHUNK = REPLACE_THREADS * REPLACE_PER;
constexpr uint32_t REPLACE_WAVES = REPLACE_THREADS / WAVE;
constexpr uint32_t REPLACE_TILE_DEFAULT = 16384, REPLACE_TILE_MIN = 256, REPLACE_TILE_MAX = 1u << 20; /* bytes of output */
constexpr uint32_t REPLACE_STAGE = 512; /* records a block holds in LDS at a time: 32 bytes each */
constexpr long long REPLACE_NEVER = 0x7FFFFFFFFFFFFFFFll, REPLACE_ALWAYS = -REPLACE_NEVER - 1;
constexpr unsigned long long REPLACE_OFF_MAX = 1ull << 56; /* table offsets beyond this are no offsets (bytes stay inside 63 bits) */

/* control words at the head of the passes' scratch, cleared in front of every call */
struct ReplaceCtl {
  unsigned int n_bad; /* records and table entries that break the contract */
  unsigned int pad[3];
};

struct ReplaceK {
  const ACMRecord *sel;            /* the selection, canonical order */
  uint64_t capacity;               /* of `sel` and the scratch arrays; the count itself when n_dev is NULL */
  const unsigned long long *n_dev; /* the record count (device), or NULL */
  const unsigned char *text;
  uint64_t n_symbols, pos_base;
  uint32_t sb;                     /* bytes per symbol of the caller's text */
  uint32_t tile_words;             /* 16-byte words per tile of pass c */
  const unsigned char *repl;       /* the table's symbols; mask mode: the fill symbol */
  const unsigned long long *repl_off; /* [n_keywords + 1] (table mode only) */
  uint64_t n_keywords;
  long long *chunk_sum;            /* [n_chunks + 1] sums of delta per chunk */
  const long long *chunk_begin;    /* [n_chunks + 1] their exclusive prefix sum: [n_chunks] = the sum of all */
  uint64_t n_chunks;
  long long *out_start;            /* [capacity] scratch */
  long long *d_out_start;          /* the caller's, or NULL */
  unsigned char *out;
  uint64_t out_capacity;
  unsigned long long *d_out_symbols;
  ReplaceCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* a scan that found more than its room left nothing to replace */
__device__ __forceinline__ bool
replace_overflowed (const ReplaceK &K) {
  return K.n_dev && *K.n_dev > K.capacity;
}

__device__ __forceinline__ uint64_t
replace_count (const ReplaceK &K) {
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  return n_raw > K.capacity ? 0 : n_raw;
}

/* record i: its start and the symbol behind it (relative to the text), its length, its replacement
 * in the table (symbols).  CHECK: against the contract, before anything else looks at the record;
 * false when it breaks it. */
template <bool MASK, bool CHECK>
__device__ __forceinline__ bool
replace_fact (const ReplaceK &K, uint64_t i, uint64_t &start, uint64_t &after, uint32_t &len, uint64_t &rbegin, uint64_t &rlen) {
  const uint4 r = *reinterpret_cast<const uint4 *> (&K.sel[i]);
  const uint64_t pos = ((uint64_t)r.y << 32) | r.x;
  len = r.z;
  if (CHECK) {
    if (record_breaks_contract (pos, len, K.pos_base, K.n_symbols))
      return false;
    if (i > 0) { /* behind the record in front of it (which answers for its own range) */
      const uint64_t prev = K.sel[i - 1].end_pos;
      if (prev < K.pos_base || prev - K.pos_base >= pos - K.pos_base + 1 - len)
        return false;
    }
  }
  after = pos - K.pos_base + 1;
  start = after - len;
  if (MASK) {
    rbegin = 0;
    rlen = len;
    return true;
  }
  if (CHECK && r.w >= K.n_keywords)
    return false;
  rbegin = K.repl_off[r.w];
  const unsigned long long rend = K.repl_off[(uint64_t)r.w + 1];
  if (CHECK && (rend < rbegin || rend > REPLACE_OFF_MAX))
    return false;
  rlen = rend - rbegin;
  return true;
}

__device__ __forceinline__ long long
replace_shfl_up (long long v, int d) {
  const uint32_t lo = __shfl_up ((uint32_t)(unsigned long long)v, d, WAVE), hi = __shfl_up ((uint32_t)((unsigned long long)v >> 32), d, WAVE);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

/* inclusive sums over the block's threads in thread order; the block's total in `total` */
__device__ __forceinline__ long long
replace_block_scan (long long v, long long *wave_sum /* [REPLACE_WAVES] LDS */, long long &total) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long o = replace_shfl_up (v, d);
    if ((int)lane >= d)
      v += o;
  }
  if (lane == WAVE - 1)
    wave_sum[wave] = v;
  __syncthreads ();
  long long before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < (int)REPLACE_WAVES; w++) {
    before += w < (int)wave ? wave_sum[w] : 0ll;
    total += wave_sum[w];
  }
  __syncthreads (); /* (the next use writes the same words) */
  return v + before;
}

/* pass a */
template <bool MASK>
__global__ __launch_bounds__ (REPLACE_THREADS) void
replace_measure_kernel (ReplaceK K) {
  __shared__ long long wave_sum[REPLACE_WAVES];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = replace_count (K);
  uint32_t bad = 0;
  if (!MASK) /* the table: offsets that never decrease, so every replacement lies in front of repl_off[n_keywords] */
    for (uint64_t k = me; k < K.n_keywords; k += stride)
      bad += K.repl_off[k] > K.repl_off[k + 1] || K.repl_off[k + 1] > REPLACE_OFF_MAX;
  for (uint64_t chunk = blockIdx.x; chunk <= K.n_chunks; chunk += gridDim.x) {
    const uint64_t base = chunk * REPLACE_CHUNK;
    long long sum = 0;
    if (chunk < K.n_chunks && base < n) { /* (uniform in the block; the prefix sum reads every entry) */
#pragma unroll
      for (int q = 0; q < (int)REPLACE_PER; q++) {
        const uint64_t i = base + (uint64_t)threadIdx.x * REPLACE_PER + q;
        if (i >= n)
          continue;
        uint64_t start, after, rbegin, rlen;
        uint32_t len;
        if (replace_fact<MASK, true> (K, i, start, after, len, rbegin, rlen))
          sum += (long long)rlen - (long long)len;
        else
          bad++;
      }
    }
    long long total;
    (void)replace_block_scan (sum, wave_sum, total);
    if (threadIdx.x == 0)
      K.chunk_sum[chunk] = total;
  }
  if (bad) {
    atomicAdd (&K.ctl->n_bad, bad);
    if (K.error)
      *K.error = 1;
  }
}

/* pass b, behind the prefix sum over the chunks */
template <bool MASK>
__global__ __launch_bounds__ (REPLACE_THREADS) void
replace_starts_kernel (ReplaceK K) {
  __shared__ long long wave_sum[REPLACE_WAVES];
  const bool stop = K.ctl->n_bad != 0 || replace_overflowed (K);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_out_symbols = stop ? 0ull : (unsigned long long)((long long)K.n_symbols + K.chunk_begin[K.n_chunks]);
  if (stop)
    return;
  const uint64_t n = replace_count (K);
  for (uint64_t chunk = blockIdx.x; chunk < K.n_chunks; chunk += gridDim.x) {
    const uint64_t base = chunk * REPLACE_CHUNK;
    if (base >= n) /* (uniform in the block) */
      break;
    uint64_t start[REPLACE_PER];
    long long delta[REPLACE_PER], mine = 0;
#pragma unroll
    for (int q = 0; q < (int)REPLACE_PER; q++) {
      const uint64_t i = base + (uint64_t)threadIdx.x * REPLACE_PER + q;
      start[q] = 0;
      delta[q] = 0;
      if (i < n) {
        uint64_t after, rbegin, rlen;
        uint32_t len;
        (void)replace_fact<MASK, false> (K, i, start[q], after, len, rbegin, rlen);
        delta[q] = (long long)rlen - (long long)len;
      }
      mine += delta[q];
    }
    long long total;
    long long at = K.chunk_begin[chunk] + replace_block_scan (mine, wave_sum, total) - mine;
#pragma unroll
    for (int q = 0; q < (int)REPLACE_PER; q++) {
      const uint64_t i = base + (uint64_t)threadIdx.x * REPLACE_PER + q;
      if (i < n) {
        const long long os = (long long)start[q] + at;
        K.out_start[i] = os;
        if (K.d_out_start)
          K.d_out_start[i] = os;
      }
      at += delta[q];
    }
  }
}

/* record j as a segment of the output, in bytes: the replacement is out[os, oe), the text goes on
 * from text[ta] at out[oe]; rb = where the replacement lies in the table.  j = -1: the front of the
 * text, in front of every record; j = n: nothing begins any more. */
struct ReplaceSeg {
  long long os, oe;
  unsigned long long ta, rb;
};

template <bool MASK>
__device__ __forceinline__ ReplaceSeg
replace_seg_global (const ReplaceK &K, long long j, uint64_t n) {
  ReplaceSeg g;
  g.ta = 0;
  g.rb = 0;
  if (j < 0) {
    g.os = REPLACE_ALWAYS;
    g.oe = 0;
    return g;
  }
  if ((uint64_t)j >= n) {
    g.os = REPLACE_NEVER;
    g.oe = REPLACE_NEVER;
    return g;
  }
  uint64_t start, after, rbegin, rlen;
  uint32_t len;
  (void)replace_fact<MASK, false> (K, (uint64_t)j, start, after, len, rbegin, rlen);
  g.os = K.out_start[j] * (long long)K.sb;
  g.oe = g.os + (long long)(rlen * K.sb);
  g.ta = after * K.sb;
  g.rb = rbegin * K.sb;
  return g;
}

/* by a whole wave: how many of a[0 .. n), which never decrease, are <= key.  64 probes a step. */
__device__ __forceinline__ uint64_t
replace_wave_count_le (const long long *a, uint64_t n, long long key) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  uint64_t lo = 0, hi = n; /* the answer lies in [lo, hi] */
  while (hi > lo) {
    const uint64_t step = (hi - lo + WAVE - 1) / WAVE;
    const uint64_t idx = lo + (uint64_t)(lane + 1) * step - 1;
    const bool le = idx < hi && a[idx] <= key;
    const uint64_t k = (uint64_t)__popcll (__ballot (le));
    const uint64_t fail = lo + (k + 1) * step - 1; /* the first probe that was greater, if there was one */
    lo += k * step;
    hi = fail < hi ? fail : hi;
  }
  return lo;
}

/* the 16 bytes at src, of any alignment: the two aligned words that hold them, shifted together */
__device__ __forceinline__ uint4
replace_load16 (const unsigned char *src) {
  const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t> (src) & 15);
  const uint4 *p = reinterpret_cast<const uint4 *> (src - r);
  const uint4 a = p[0];
  uint4 b = a;
  if (r)
    b = p[1]; /* (holds src[15]) */
  const uint32_t q = r >> 2, sh = (r & 3) * 8;
  const uint32_t e0 = q == 0 ? a.x : q == 1 ? a.y : q == 2 ? a.z : a.w;
  const uint32_t e1 = q == 0 ? a.y : q == 1 ? a.z : q == 2 ? a.w : b.x;
  const uint32_t e2 = q == 0 ? a.z : q == 1 ? a.w : q == 2 ? b.x : b.y;
  const uint32_t e3 = q == 0 ? a.w : q == 1 ? b.x : q == 2 ? b.y : b.z;
  const uint32_t e4 = q == 0 ? b.x : q == 1 ? b.y : q == 2 ? b.z : b.w;
  uint4 v;
  v.x = (uint32_t)((((uint64_t)e1 << 32) | e0) >> sh);
  v.y = (uint32_t)((((uint64_t)e2 << 32) | e1) >> sh);
  v.z = (uint32_t)((((uint64_t)e3 << 32) | e2) >> sh);
  v.w = (uint32_t)((((uint64_t)e4 << 32) | e3) >> sh);
  return v;
}

/* LDS of replace_build_kernel: the staged records [pf, pf + cnt) and the start of the one behind them */
struct ReplaceStage {
  long long os[REPLACE_STAGE + 1], oe[REPLACE_STAGE];
  unsigned long long ta[REPLACE_STAGE], rb[REPLACE_STAGE];
};

/* record j and where the record behind it begins: from the stage when it is there */
template <bool MASK>
__device__ __forceinline__ ReplaceSeg
replace_seg (const ReplaceK &K, const ReplaceStage &S, long long pf, uint32_t cnt, long long j, uint64_t n, long long &next) {
  if (j >= pf && j < pf + (long long)cnt) {
    const uint32_t i = (uint32_t)(j - pf);
    ReplaceSeg g;
    g.os = S.os[i];
    g.oe = S.oe[i];
    g.ta = S.ta[i];
    g.rb = S.rb[i];
    next = S.os[i + 1];
    return g;
  }
  next = replace_seg_global<MASK> (K, j + 1, n).os;
  return replace_seg_global<MASK> (K, j, n);
}

/* pass c */
template <bool MASK>
__global__ __launch_bounds__ (REPLACE_THREADS) void
replace_build_kernel (ReplaceK K) {
  __shared__ ReplaceStage S;
  __shared__ long long s_first, s_end;
  if (K.ctl->n_bad != 0 || replace_overflowed (K))
    return;
  const uint64_t n = replace_count (K);
  const uint32_t sb = K.sb;
  const unsigned long long out_symbols = *K.d_out_symbols;
  /* (an output that has no room: what there is room for is written, the caller sees the need) */
  const long long total = (long long)((out_symbols < K.out_capacity ? out_symbols : K.out_capacity) * sb);
  if (total <= 0)
    return;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t> (K.out) & 15);
  uint4 *const grid = reinterpret_cast<uint4 *> (K.out - mis); /* word w = out[16 w - mis, 16 w - mis + 16) */
  const long long n_words = (total + mis + 15) / 16, TW = K.tile_words;
  const long long tiles = (n_words + TW - 1) / TW;
  uint4 fill = make_uint4 (0, 0, 0, 0);
  if (MASK) { /* (the buffers' addresses are multiples of sb, and sb divides 16: byte t of every word is byte t % sb of the symbol) */
    uint32_t f[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int t = 0; t < 16; t++)
      f[t / 4] |= (uint32_t)K.repl[t & (sb - 1)] << (8 * (t % 4));
    fill = make_uint4 (f[0], f[1], f[2], f[3]);
  }
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long w0 = tile * TW, w1 = w0 + TW < n_words ? w0 + TW : n_words;
    const long long lo_b = w0 * 16 > mis ? w0 * 16 - mis : 0;         /* the tile's bytes of the output */
    const long long hi_b = w1 * 16 - mis < total ? w1 * 16 - mis : total;
    if (threadIdx.x < WAVE) { /* the last record that begins at or in front of the tile's first byte (-1: none), and
                               * the records that begin in front of its end: no other is staged */
      const uint64_t c = replace_wave_count_le (K.out_start, n, lo_b / (long long)sb);
      const uint64_t c_end = replace_wave_count_le (K.out_start, n, (hi_b - 1) / (long long)sb);
      if (threadIdx.x == 0) {
        s_first = (long long)c - 1;
        s_end = (long long)c_end;
      }
    }
    __syncthreads ();
    long long pf = s_first, piece_lo = lo_b;
    const long long pe = s_end; /* pf < pe <= n: the record in front of the tile counts as one that touches it */
    bool first_piece = true;
    for (;;) { /* (everything that steers this loop is uniform in the block) */
      const uint64_t left = (uint64_t)(pe - pf);
      const uint32_t cnt = left < REPLACE_STAGE ? (uint32_t)left : REPLACE_STAGE; /* at least 1 */
      for (uint32_t i = threadIdx.x; i <= cnt; i += blockDim.x) {
        const ReplaceSeg g = replace_seg_global<MASK> (K, pf + i, n);
        S.os[i] = g.os;
        if (i < cnt) {
          S.oe[i] = g.oe;
          S.ta[i] = g.ta;
          S.rb[i] = g.rb;
        }
      }
      __syncthreads ();
      /* this piece makes the words whose first byte of the output lies in [piece_lo, piece_hi) */
      const long long behind = S.os[cnt];
      const long long piece_hi = behind < hi_b ? behind : hi_b;
      const long long wa = first_piece ? w0 : (piece_lo + mis + 15) / 16;
      long long wb = (piece_hi + mis + 15) / 16;
      wb = wb < w1 ? wb : w1;
      for (long long w = wa + threadIdx.x; w < wb; w += blockDim.x) {
        const long long b0 = w * 16 - mis, kb = b0 > 0 ? b0 : 0;
        uint32_t l = 0, h = cnt - 1; /* the last staged record that begins at or in front of kb: S.os[0] <= kb */
        while (l < h) {
          const uint32_t mid = (l + h + 1) / 2;
          if (S.os[mid] <= kb)
            l = mid;
          else
            h = mid - 1;
        }
        const long long os = S.os[l], oe = S.oe[l], nxt = S.os[l + 1];
        const bool whole = b0 >= 0 && b0 + 16 <= total;
        if (whole && b0 + 16 <= oe) { /* inside one replacement */
          grid[w] = MASK ? fill : replace_load16 (K.repl + S.rb[l] + (unsigned long long)(b0 - os));
        } else if (whole && b0 >= oe && b0 + 16 <= nxt) { /* inside one stretch of text: nearly every word of a log */
          grid[w] = replace_load16 (K.text + S.ta[l] + (unsigned long long)(b0 - oe));
        } else { /* across a boundary, or the first or last word of a buffer off the grid: byte by byte */
          long long j = pf + l, next = nxt;
          ReplaceSeg g;
          g.os = os;
          g.oe = oe;
          g.ta = S.ta[l];
          g.rb = S.rb[l];
          uint32_t v[4] = { 0, 0, 0, 0 };
          const uint32_t fw[4] = { fill.x, fill.y, fill.z, fill.w };
#pragma unroll
          for (int t = 0; t < 16; t++) {
            const long long b = b0 + t;
            if (b < 0 || b >= total)
              continue;
            while (b >= next) { /* (records that delete their match begin where the next one does) */
              j++;
              g = replace_seg<MASK> (K, S, pf, cnt, j, n, next);
            }
            uint32_t byte;
            if (b < g.oe)
              byte = MASK ? (fw[t / 4] >> (8 * (t % 4))) & 0xFFu : K.repl[g.rb + (unsigned long long)(b - g.os)];
            else
              byte = K.text[g.ta + (unsigned long long)(b - g.oe)];
            v[t / 4] |= byte << (8 * (t % 4));
          }
          if (whole)
            grid[w] = make_uint4 (v[0], v[1], v[2], v[3]);
          else {
#pragma unroll
            for (int t = 0; t < 16; t++)
              if (b0 + t >= 0 && b0 + t < total)
                K.out[b0 + t] = (unsigned char)(v[t / 4] >> (8 * (t % 4)));
          }
        }
      }
      __syncthreads (); /* (the next piece, or the next tile, goes into the same LDS) */
      if (pf + (long long)cnt >= pe) /* (the record behind the last one staged begins at or behind the tile's end) */
        break;
      piece_lo = behind;
      pf += cnt;
      first_piece = false;
    }
  }
}
