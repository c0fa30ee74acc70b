/* dev_context.h -- match contexts: CONTEXT of a record set, the text around the matches gathered
 * into snippets (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * CONTEXT is a function of the records and of offsets[]: no pass looks at the text before the
 * gather, and no pass is proportional to the text -- a record's text is a bisection of offsets[]
 * (WORDS' way: no index over the buffer, so the scratch is sized by the records alone).  Tiles of
 * K.tile records (a multiple of 64), blocks stride over the tiles, a block takes CONTEXT_THREADS
 * records of its tile at a time.  Behind offsets_check_kernel (dev_batch.h; offsets[] given: the batch contract,
 * in a launch of its own so that no address is formed from an offset the check has not seen):
 *   1. context_window_kernel: a lane takes CONTEXT_PER records 256 apart, validates them (WORDS' test;
 *      under MERGE also that end_pos does not decrease from the record in front), finds their texts --
 *      the bisections step together, so that their probes are loads in flight side by side and not
 *      one chain of log2 n_texts dependent loads behind the other -- and writes every window [lo, hi)
 *      and its text to scratch; a record that spans a cut is marked windowless.  Per tile:
 *      EACH -- the sum of the window lengths; MERGE -- the minimum of lo and the maximum of hi.
 *   MERGE.  Over the windowed records hi never decreases (end_pos does not, and a windowed record
 *   ends in the text it begins in), lo can.  Record j begins a snippet iff the minimum of lo over j
 *   and every later windowed record exceeds hi_prev, the hi of the windowed record in front of j
 *   (none: it begins one), or -- SYMBOLS -- hi_prev <= offsets[t_j]: the text changed.  That
 *   snippet's first symbol is the same suffix minimum.
 *   2. context_carry_kernel, one block: the tiles' maxima become prefix maxima and the tiles' minima
 *      suffix minima, in place (a serial walk of 256 tiles a step over 8 bytes per 4,096 records).
 *   3. context_flag_kernel: inside every tile the suffix minimum of lo (backwards, carried in from
 *      the tiles behind) replaces lo[], hi_prev (forwards, carried in from the tiles in front)
 *      replaces hi[]; the tile's number of begins and the sum of d_j = hi_prev - lo_j over its
 *      begins (signed, hi_prev = 0 for the first).  With S_j the sum of d over the begins up to and
 *      including j, snippet q that begins at j lies at out_offsets[q] = S_j + lo_j: the sum
 *      telescopes to the lengths of the snippets in front.
 *   4. two exclusive sums over the tiles (hipCUB, 64-bit), then context_index_kernel: the scans
 *      inside the tiles; n_snippets, out_symbols, snip_lo[], out_offsets[], snip_text[], rec_snip[]
 *      and rec_at[i] = S_i + s_i (MERGE), = out_offsets[i] + s_i - lo_i (EACH).
 *   5. context_gather_kernel (only with an output buffer), output-stationary: grep_gather_kernel's
 *      copy with (snip_lo, out_offsets) in place of (kept text, kept_off) -- tiles of whole 16-byte
 *      words of the OUTPUT buffer's own grid, a bisection of out_offsets[] per word, replace_load16
 *      for a word inside one snippet, byte by byte across a boundary and off the grid.  Every output
 *      byte is written once, by one lane; no atomics.  It returns at once when the output has no room.
 * A contract violation (offsets, a record, the order under MERGE) is noted in ContextCtl by
 * passes that form no address from what they check; every later pass then returns at once, the two
 * counts are 0.  The aligned loads of the gather may take in up to 15 bytes in front of or behind the
 * snippet they copy: bytes of a 16-byte word that holds a byte of it, so of the same page.
 * Launch geometry never depends on what the records hold: capped grids, grid-stride loops. */
constexpr uint32_t CONTEXT_THREADS = 256, CONTEXT_WAVES = CONTEXT_THREADS / WAVE;
constexpr uint32_t CONTEXT_PER = 4; /* records of a lane whose text searches run side by side in pass 1 */
constexpr uint32_t CONTEXT_TILE_DEFAULT = 4096, CONTEXT_TILE_MIN = 64, CONTEXT_TILE_MAX = 1u << 20;           /* records */
constexpr uint32_t CONTEXT_OUT_TILE_DEFAULT = 16384, CONTEXT_OUT_TILE_MIN = 256, CONTEXT_OUT_TILE_MAX = 1u << 20; /* bytes of output */
constexpr unsigned long long CONTEXT_NEVER = ~0ull;
constexpr uint32_t CONTEXT_WINDOWLESS = 1u << 31; /* in tx[]: the record spans a cut (a text is below 2^31) */
static_assert (CONTEXT_THREADS == REPLACE_THREADS, "replace_wave_count_le and replace_shfl_up are shared");

/* control words at the head of the passes' scratch, cleared in front of every call */
struct ContextCtl {
  unsigned long long n; /* records the passes work on (0 after an overflow and under bad offsets) */
  unsigned int bad;     /* offsets[] break the batch contract (offsets_check_kernel) */
  unsigned int n_bad;   /* records that break the contract, or the order under MERGE (pass 1) */
  unsigned int over;    /* *d_n > capacity: a scan that overflowed */
  unsigned int pad;
};

struct ContextK {
  const unsigned char *text;       /* the caller's pointer: any multiple of sb */
  uint64_t n_symbols, pos_base;
  const uint64_t *offsets;         /* [n_texts + 1], NULL: one text */
  uint64_t n_texts;
  const ACMRecord *in;             /* MERGE: end_pos never decreases */
  uint64_t capacity;               /* of `in` and the per-record arrays; the count itself when n_dev is NULL */
  const unsigned long long *n_dev; /* the record count (device), or NULL */
  uint32_t before, after, flags;   /* ACM_CONTEXT_* */
  uint32_t tile;                   /* records per tile, a multiple of WAVE */
  uint64_t n_tiles;                /* tiles of `capacity` records */
  unsigned long long *lo, *hi;     /* [capacity] scratch: the windows; behind pass 3 the suffix minimum and hi_prev */
  uint32_t *tx;                    /* [capacity] scratch: the records' texts | CONTEXT_WINDOWLESS */
  unsigned long long *tile_lo, *tile_hi; /* [n_tiles + 1] MERGE: minimum of lo ([n_tiles] stays NEVER), maximum of hi per tile */
  long long *tile_cnt, *tile_sum;  /* [n_tiles + 1] begins (MERGE) and the sum of d (MERGE) or of the lengths (EACH) per tile */
  const long long *tile_cnt_begin, *tile_sum_begin; /* [n_tiles + 1] their exclusive prefix sums: [n_tiles] = the sum of all */
  unsigned long long *d_n_snippets, *d_out_symbols;
  unsigned long long *d_snip_lo;   /* [capacity] */
  long long *d_out_offsets;        /* [capacity + 1] */
  uint32_t *d_snip_text, *d_rec_snip; /* [capacity], each may be NULL */
  long long *d_rec_at;             /* [capacity], may be NULL */
  unsigned char *out;
  uint64_t out_capacity;
  uint32_t sb;                     /* bytes per symbol of the caller's text */
  uint32_t tile_words;             /* 16-byte words per tile of pass 5 */
  ContextCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* the call reports nothing */
__device__ __forceinline__ bool
context_stopped (const ContextK &K) {
  return K.ctl->bad != 0 || K.ctl->n_bad != 0 || K.ctl->over != 0;
}

enum { CONTEXT_MIN, CONTEXT_MAX, CONTEXT_ADD };

template <int OP>
__device__ __forceinline__ unsigned long long
context_op (unsigned long long a, unsigned long long b) {
  if (OP == CONTEXT_MIN)
    return a < b ? a : b;
  if (OP == CONTEXT_MAX)
    return a > b ? a : b;
  return a + b; /* (signed sums wrap the same way) */
}

/* OP over the values of the threads in front of this one, in thread order (the neutral element for
 * thread 0), and over the whole block in `total` */
template <int OP>
__device__ __forceinline__ unsigned long long
context_block_scan (unsigned long long v, unsigned long long *wave_val /* [CONTEXT_WAVES] LDS */, unsigned long long &total) {
  const unsigned long long neutral = OP == CONTEXT_MIN ? CONTEXT_NEVER : 0ull;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const unsigned long long o = (unsigned long long)replace_shfl_up ((long long)v, d);
    if ((int)lane >= d)
      v = context_op<OP> (o, v);
  }
  if (lane == WAVE - 1)
    wave_val[wave] = v;
  unsigned long long front = (unsigned long long)replace_shfl_up ((long long)v, 1);
  if (lane == 0)
    front = neutral;
  __syncthreads ();
  unsigned long long waves_front = neutral;
  total = neutral;
#pragma unroll
  for (int w = 0; w < (int)CONTEXT_WAVES; w++) {
    waves_front = w < (int)wave ? context_op<OP> (waves_front, wave_val[w]) : waves_front;
    total = context_op<OP> (total, wave_val[w]);
  }
  __syncthreads (); /* (the next use writes the same words) */
  return context_op<OP> (waves_front, front);
}

/* batch_text_of for PER positions at once, from the whole of offsets[]: a fixed number of steps (a
 * range of R + 1 texts is one of at most R / 2 + 1 after a step; a range that has closed stays
 * closed: mid = lo, offsets[lo] <= pos), so that the PER probes of a step are independent loads in
 * flight together and not PER chains one behind the other */
template <int PER>
__device__ __forceinline__ void
context_texts_of (const ContextK &K, const uint64_t (&pos)[PER], uint64_t (&t)[PER]) {
  uint64_t hi[PER];
#pragma unroll
  for (int q = 0; q < PER; q++) {
    t[q] = 0;
    hi[q] = K.n_texts - 1;
  }
  for (uint64_t span = K.n_texts - 1; span; span >>= 1) { /* (uniform) */
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const uint64_t mid = t[q] + (hi[q] - t[q] + 1) / 2;
      const bool le = K.offsets[mid] <= pos[q];
      t[q] = le ? mid : t[q];
      hi[q] = le ? hi[q] : mid - 1;
    }
  }
}

/* record r against the contract: its start and its end relative to the buffer, 0 <= s <= e < n_symbols */
__device__ __forceinline__ bool
context_record (const ContextK &K, const uint4 r, uint64_t &s, uint64_t &e) {
  const uint64_t pos = ((uint64_t)r.y << 32) | r.x;
  s = e = 0;
  if (record_breaks_contract (pos, r.z, K.pos_base, K.n_symbols))
    return false;
  e = pos - K.pos_base;
  s = e + 1 - r.z;
  return true;
}

/* the window of the record [s, e] of text t.  tx = t, with CONTEXT_WINDOWLESS when the record spans a
 * cut: then lo = hi = its start. */
__device__ __forceinline__ void
context_window (const ContextK &K, uint64_t s, uint64_t e, uint64_t t, unsigned long long &lo, unsigned long long &hi, uint32_t &tx) {
  uint64_t t_lo = 0, t_hi = K.n_symbols; /* the record's text: [t_lo, t_hi) */
  if (K.offsets) { /* (uniform; checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols) */
    t_lo = K.offsets[t];
    t_hi = K.offsets[t + 1];
    if (e >= t_hi) { /* the match spans a cut: no match of any text */
      lo = hi = s;
      tx = (uint32_t)t | CONTEXT_WINDOWLESS;
      return;
    }
  }
  tx = (uint32_t)t;
  if (K.flags & ACM_CONTEXT_TEXTS) { /* (offsets given: the host has refused the call otherwise) */
    lo = K.offsets[t > K.before ? t - K.before : 0];
    hi = K.offsets[K.n_texts - (t + 1) > K.after ? t + 1 + K.after : K.n_texts];
  } else {
    lo = s - t_lo > K.before ? s - K.before : t_lo;
    hi = t_hi - (e + 1) > K.after ? e + 1 + K.after : t_hi;
  }
}

/* pass 1 */
template <bool MERGE>
__global__ __launch_bounds__ (CONTEXT_THREADS) void
context_window_kernel (ContextK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  const uint64_t n = n_raw > K.capacity || K.ctl->bad ? 0 : n_raw; /* an overflowing scan left nothing to show */
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    K.ctl->n = n;
    K.ctl->over = n_raw > K.capacity ? 1u : 0u;
  }
  uint32_t bad = 0;
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    unsigned long long mn = CONTEXT_NEVER, mx = 0, sum = 0;
    if (tile < K.n_tiles && base < n) { /* (uniform in the block; the scans behind read every entry) */
      const uint64_t end = base + K.tile < n ? base + K.tile : n;
      for (uint64_t i0 = base + threadIdx.x; i0 < end; i0 += CONTEXT_THREADS * CONTEXT_PER) { /* CONTEXT_PER records of a lane in flight */
        uint64_t s[CONTEXT_PER], e[CONTEXT_PER], t[CONTEXT_PER];
        bool ok[CONTEXT_PER];
#pragma unroll
        for (int q = 0; q < (int)CONTEXT_PER; q++) {
          const uint64_t i = i0 + (uint64_t)q * CONTEXT_THREADS;
          ok[q] = false;
          s[q] = e[q] = t[q] = 0;
          if (i < end) {
            const uint4 r = *reinterpret_cast<const uint4 *> (&K.in[i]);
            ok[q] = context_record (K, r, s[q], e[q]);
            bad += ok[q] ? 0u : 1u;
            if (MERGE && i > 0 && K.in[i - 1].end_pos > ((((uint64_t)r.y) << 32) | r.x))
              bad++;
          }
        }
        if (K.offsets) /* (a record that is none, or breaks the contract, looks for position 0: in bounds, not used) */
          context_texts_of<CONTEXT_PER> (K, s, t);
        unsigned long long lo[CONTEXT_PER], hi[CONTEXT_PER];
        uint32_t tx[CONTEXT_PER];
#pragma unroll
        for (int q = 0; q < (int)CONTEXT_PER; q++) {
          lo[q] = hi[q] = 0;
          tx[q] = CONTEXT_WINDOWLESS;
          if (ok[q])
            context_window (K, s[q], e[q], t[q], lo[q], hi[q], tx[q]);
        }
#pragma unroll
        for (int q = 0; q < (int)CONTEXT_PER; q++) {
          const uint64_t i = i0 + (uint64_t)q * CONTEXT_THREADS;
          if (i >= end)
            continue;
          K.lo[i] = lo[q];
          K.hi[i] = hi[q];
          K.tx[i] = tx[q];
          if (!(tx[q] & CONTEXT_WINDOWLESS)) {
            mn = lo[q] < mn ? lo[q] : mn;
            mx = hi[q] > mx ? hi[q] : mx;
            sum += hi[q] - lo[q];
          }
        }
      }
    }
    unsigned long long all;
    if (MERGE) {
      (void)context_block_scan<CONTEXT_MIN> (mn, wave_val, all);
      if (threadIdx.x == 0)
        K.tile_lo[tile] = all;
      (void)context_block_scan<CONTEXT_MAX> (mx, wave_val, all);
      if (threadIdx.x == 0)
        K.tile_hi[tile] = all;
    } else {
      (void)context_block_scan<CONTEXT_ADD> (sum, wave_val, all);
      if (threadIdx.x == 0)
        K.tile_sum[tile] = (long long)all;
    }
  }
  if (bad) {
    atomicAdd (&K.ctl->n_bad, bad);
    if (K.error)
      *K.error = 1;
  }
}

/* pass 2 (MERGE), one block: tile_hi[i] = the maximum over the tiles up to i, tile_lo[i] = the
 * minimum over the tiles from i on, in place */
__global__ __launch_bounds__ (CONTEXT_THREADS) void
context_carry_kernel (ContextK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  if (context_stopped (K))
    return;
  unsigned long long carry = 0, all;
  for (uint64_t base = 0; base < K.n_tiles; base += CONTEXT_THREADS) { /* (uniform in the block) */
    const uint64_t i = base + threadIdx.x;
    const unsigned long long v = i < K.n_tiles ? K.tile_hi[i] : 0ull;
    const unsigned long long front = context_block_scan<CONTEXT_MAX> (v, wave_val, all);
    if (i < K.n_tiles)
      K.tile_hi[i] = context_op<CONTEXT_MAX> (carry, context_op<CONTEXT_MAX> (front, v));
    carry = context_op<CONTEXT_MAX> (carry, all);
  }
  carry = CONTEXT_NEVER;
  for (uint64_t base = 0; base < K.n_tiles; base += CONTEXT_THREADS) { /* thread order is descending tile order */
    const bool in = base + threadIdx.x < K.n_tiles;
    const uint64_t i = K.n_tiles - 1 - (base + threadIdx.x);
    const unsigned long long v = in ? K.tile_lo[i] : CONTEXT_NEVER;
    const unsigned long long front = context_block_scan<CONTEXT_MIN> (v, wave_val, all);
    if (in)
      K.tile_lo[i] = context_op<CONTEXT_MIN> (carry, context_op<CONTEXT_MIN> (front, v));
    carry = context_op<CONTEXT_MIN> (carry, all);
  }
}

/* MERGE: windowed record of text t begins a snippet; low = the minimum of lo from the record on,
 * hi_prev = the hi of the windowed record in front of it (0: none, a window ends behind symbol 0) */
__device__ __forceinline__ bool
context_begins (const ContextK &K, uint32_t t, unsigned long long low, unsigned long long hi_prev) {
  if (hi_prev == 0 || low > hi_prev)
    return true;
  return !(K.flags & ACM_CONTEXT_TEXTS) && K.offsets && hi_prev <= K.offsets[t]; /* (a window of text t ends behind offsets[t]) */
}

/* pass 3 (MERGE) */
__global__ __launch_bounds__ (CONTEXT_THREADS) void
context_flag_kernel (ContextK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  const bool stop = context_stopped (K);
  const uint64_t n = K.ctl->n;
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    unsigned long long cnt = 0, sum = 0, all;
    if (!stop && tile < K.n_tiles && base < n) { /* (uniform in the block; the sums behind read every entry) */
      const uint64_t end = base + K.tile < n ? base + K.tile : n;
      const uint64_t steps = (end - base + CONTEXT_THREADS - 1) / CONTEXT_THREADS;
      unsigned long long carry = K.tile_lo[tile + 1]; /* backwards: thread order is descending record order */
      for (uint64_t k = steps; k-- > 0;) {
        const uint64_t i = base + k * CONTEXT_THREADS + (CONTEXT_THREADS - 1 - threadIdx.x);
        const unsigned long long v = i < end && !(K.tx[i] & CONTEXT_WINDOWLESS) ? K.lo[i] : CONTEXT_NEVER;
        const unsigned long long front = context_block_scan<CONTEXT_MIN> (v, wave_val, all);
        if (i < end)
          K.lo[i] = context_op<CONTEXT_MIN> (carry, context_op<CONTEXT_MIN> (front, v));
        carry = context_op<CONTEXT_MIN> (carry, all);
      }
      carry = tile ? K.tile_hi[tile - 1] : 0ull;
      for (uint64_t k = 0; k < steps; k++) {
        const uint64_t i = base + k * CONTEXT_THREADS + threadIdx.x;
        const uint32_t tx = i < end ? K.tx[i] : CONTEXT_WINDOWLESS;
        const unsigned long long v = tx & CONTEXT_WINDOWLESS ? 0ull : K.hi[i];
        const unsigned long long hi_prev = context_op<CONTEXT_MAX> (carry, context_block_scan<CONTEXT_MAX> (v, wave_val, all));
        if (i < end)
          K.hi[i] = hi_prev;
        if (!(tx & CONTEXT_WINDOWLESS) && context_begins (K, tx, K.lo[i], hi_prev)) {
          cnt++;
          sum += hi_prev - K.lo[i];
        }
        carry = context_op<CONTEXT_MAX> (carry, all);
      }
    }
    (void)context_block_scan<CONTEXT_ADD> (cnt, wave_val, all);
    if (threadIdx.x == 0)
      K.tile_cnt[tile] = (long long)all;
    (void)context_block_scan<CONTEXT_ADD> (sum, wave_val, all);
    if (threadIdx.x == 0)
      K.tile_sum[tile] = (long long)all;
  }
}

/* pass 4, behind the prefix sums over the tiles */
template <bool MERGE>
__global__ __launch_bounds__ (CONTEXT_THREADS) void
context_index_kernel (ContextK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  const bool stop = context_stopped (K);
  const uint64_t n = K.ctl->n;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    /* (MERGE: the sum of d and the end of the last snippet, the largest hi of all) */
    const unsigned long long n_snippets = stop ? 0ull : MERGE ? (unsigned long long)K.tile_cnt_begin[K.n_tiles] : n;
    const unsigned long long all =
      stop ? 0ull : (unsigned long long)K.tile_sum_begin[K.n_tiles] + (MERGE && K.n_tiles ? K.tile_hi[K.n_tiles - 1] : 0ull);
    *K.d_n_snippets = n_snippets;
    *K.d_out_symbols = all;
    if (!stop)
      K.d_out_offsets[n_snippets] = (long long)all;
  }
  if (stop) /* every other output stays as it was */
    return;
  const bool texts = (K.flags & ACM_CONTEXT_TEXTS) != 0;
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) */
      break;
    const uint64_t end = base + K.tile < n ? base + K.tile : n;
    unsigned long long at_cnt = MERGE ? (unsigned long long)K.tile_cnt_begin[tile] : 0ull, at_sum = (unsigned long long)K.tile_sum_begin[tile];
    for (uint64_t step = base; step < end; step += CONTEXT_THREADS) { /* (uniform in the block) */
      const uint64_t i = step + threadIdx.x;
      const uint32_t tx = i < end ? K.tx[i] : CONTEXT_WINDOWLESS;
      const bool windowed = !(tx & CONTEXT_WINDOWLESS);
      const uint32_t t = tx & ~CONTEXT_WINDOWLESS;
      unsigned long long lo = 0, s = 0, cnt = 0, add = 0, all;
      if (i < end) {
        const ACMRecord r = K.in[i];
        lo = K.lo[i];
        s = r.end_pos - K.pos_base + 1 - r.length;
        if (!MERGE)
          add = K.hi[i] - lo;
        else if (windowed && context_begins (K, t, lo, K.hi[i])) {
          cnt = 1;
          add = K.hi[i] - lo;
        }
      }
      unsigned long long q = i, sum = at_sum + context_block_scan<CONTEXT_ADD> (add, wave_val, all); /* EACH: where snippet i lies */
      at_sum += all;
      if (MERGE) {
        sum += add; /* S_i */
        q = at_cnt + context_block_scan<CONTEXT_ADD> (cnt, wave_val, all) + cnt - 1;
        at_cnt += all;
      }
      if (i >= end)
        continue;
      if (MERGE ? cnt != 0 : true) {
        K.d_snip_lo[q] = lo;
        K.d_out_offsets[q] = (long long)(MERGE ? sum + lo : sum);
        if (K.d_snip_text) /* the text that holds lo: under TEXTS the first text of the window that has a symbol */
          K.d_snip_text[q] = texts && windowed ? (uint32_t)batch_text_of (K.offsets, t > K.before ? t - K.before : 0, t, lo) : t;
      }
      if (K.d_rec_snip)
        K.d_rec_snip[i] = windowed ? (uint32_t)q : 0xFFFFFFFFu;
      if (K.d_rec_at)
        K.d_rec_at[i] = windowed ? (long long)(MERGE ? sum + s : sum + s - lo) : -1ll;
    }
  }
}

/* pass 5 */
__global__ __launch_bounds__ (CONTEXT_THREADS) void
context_gather_kernel (ContextK K) {
  __shared__ long long s_first, s_last;
  const unsigned long long out_symbols = *K.d_out_symbols;
  if (out_symbols == 0 || out_symbols > K.out_capacity) /* nothing to show, or no room: the caller sees the need, nothing is written */
    return;
  const uint64_t n_snippets = *K.d_n_snippets;
  const long long sb = K.sb;
  const long long total = (long long)out_symbols * sb;
  const long long *const koff = K.d_out_offsets; /* [n_snippets + 1], never decreasing, [n_snippets] = out_symbols */
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t> (K.out) & 15);
  uint4 *const grid = reinterpret_cast<uint4 *> (K.out - mis); /* word w = out[16 w - mis, 16 w - mis + 16) */
  const long long n_words = (total + mis + 15) / 16, TW = K.tile_words;
  const long long tiles = (n_words + TW - 1) / TW;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long w0 = tile * TW, w1 = w0 + TW < n_words ? w0 + TW : n_words;
    const long long lo_b = w0 * 16 > mis ? w0 * 16 - mis : 0; /* the tile's bytes of the output */
    const long long hi_b = w1 * 16 - mis < total ? w1 * 16 - mis : total;
    if (threadIdx.x < WAVE) { /* the snippets that hold the tile's first and last symbol: koff[0] = 0 and koff[n_snippets] lies
                               * behind every symbol, so both counts lie in [1, n_snippets]; of empty snippets (EACH, a windowless
                               * record) that begin at the same place the last one counts */
      const uint64_t c = replace_wave_count_le (koff, n_snippets + 1, lo_b / sb);
      const uint64_t c_end = replace_wave_count_le (koff, n_snippets + 1, (hi_b - 1) / sb);
      if (threadIdx.x == 0) {
        s_first = (long long)c - 1;
        s_last = (long long)c_end - 1;
      }
    }
    __syncthreads ();
    const long long jf = s_first, jl = s_last;
    for (long long w = w0 + threadIdx.x; w < w1; w += blockDim.x) {
      const long long b0 = w * 16 - mis, kb = b0 > 0 ? b0 : 0;
      const long long s = kb / sb;
      long long l = jf, h = jl; /* the last snippet that begins at or in front of symbol s: koff[jf] <= s */
      while (l < h) {
        const long long mid = (l + h + 1) / 2;
        if (koff[mid] <= s)
          l = mid;
        else
          h = mid - 1;
      }
      long long j = l, os = koff[j] * sb, oe = koff[j + 1] * sb;
      const unsigned char *src = K.text + K.d_snip_lo[j] * (uint64_t)sb;
      const bool whole = b0 >= 0 && b0 + 16 <= total;
      if (whole && b0 + 16 <= oe) { /* inside one snippet */
        grid[w] = replace_load16 (src + (b0 - os));
      } else { /* across a boundary, or the first or last word of a buffer off the grid: byte by byte */
        uint32_t v[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int t = 0; t < 16; t++) {
          const long long b = b0 + t;
          if (b < 0 || b >= total)
            continue;
          if (b >= oe) {
            do { /* (b < total = koff[n_snippets] * sb: the walk ends at a snippet in front of n_snippets) */
              j++;
              os = oe;
              oe = koff[j + 1] * sb;
            } while (b >= oe);
            src = K.text + K.d_snip_lo[j] * (uint64_t)sb;
          }
          v[t / 4] |= (uint32_t)src[b - os] << (8 * (t % 4));
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
    __syncthreads (); /* (the next tile's bounds go into the same words) */
  }
}
