/* dev_grep.h -- grep over a batch: how many matches every text has, which texts have one (or none),
 * and those texts gathered into a new packed buffer (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * hits[t] of a batch is a histogram of the TEXTS of its records, as the tally is one of their
 * keywords: the record scan of any plan kind (no scan kernel touched), window by window into a
 * record area of `capacity` records in the caller's scratch, and one pass over what every window
 * found.  The passes, all on the caller's stream:
 *   1. batch_index_kernel<false> (dev_batch.h), once, in front of the windows: the contract on
 *      offsets[] and the text that holds the first position of every block of 4,096 positions.  No
 *      later pass forms an address from an offset when it has raised GrepCtl::batch.bad.
 *   2. grep_hits_kernel, behind every window's scan: reads the window's record count on the device,
 *      atomicMax into GrepCtl::need and nothing else when this or an earlier window held more than
 *      `capacity` (the tally's protocol).  Else a grid-stride loop over the records in whatever
 *      order the scan left them, one 16-byte load per lane: the position, rebased from the window's
 *      read begin to the buffer; its text through the index (batch_text_of between the index
 *      entries of its block and the next); kept iff the match begins inside that text
 *      (batch_filter_kernel's test); one add to hits[text], a SCRATCH array of 64-bit counters.
 *      A window of matches in one long text would put every lane on one address: the lanes of a
 *      wave that hold the text of the wave's first kept lane add ONCE (two ballots, a popcount, one
 *      atomic by one lane); the lanes that hold another text add for themselves.  A position
 *      outside the buffer raises the plan's error flag and is not counted.
 *   3. grep_flag_kernel, COUNT then WRITE, over tiles of GREP_TILE consecutive texts: a text is
 *      KEPT iff (hits[t] > 0) != INVERT.  COUNT: the tile's kept texts (32-bit) and their symbols
 *      (64-bit), and the sum of all hits into GrepCtl::total; two exclusive prefix sums over the
 *      tiles (hipCUB) between; WRITE: the same walk, rank by ballot within the wave and by the
 *      waves' counts in LDS within the block -- stable, ascending -- and the same for the symbols
 *      with a shuffle scan: kept[], out_offsets[] (to scratch for pass 4 and to the caller's
 *      arrays), hits[] to the caller, and the call's scalars.
 *   4. grep_gather_kernel (only with an output buffer), output-stationary as replace_build_kernel
 *      is: the output is cut into tiles of whole 16-byte words of the OUTPUT buffer's own grid.  A
 *      block finds the first and the last kept text that touch its tile (two 64-way searches of a
 *      wave over out_offsets[]); every lane makes whole words: a bisection of out_offsets[] between
 *      those two finds the kept text of the word's first byte; a word that lies inside one text
 *      loads the two aligned source words that hold it and shifts them together
 *      (replace_load16); a word that straddles a text boundary is put together byte by byte,
 *      stepping to the next kept text where one ends.  One 16-byte store per word; the first and
 *      the last word of an output off the grid go by byte stores.  Every output byte is written
 *      once, by one lane; no atomics.  It returns at once when the output has no room, on a record
 *      overflow or on bad offsets.
 * The aligned loads of the fast path may take in up to 15 bytes in front of or behind the text they
 * copy: bytes of a 16-byte word that holds a byte of the text, so of the same page.
 * Launch geometry never depends on the number of texts or of records: capped grids, grid-stride
 * loops. */
constexpr uint32_t GREP_THREADS = 256, GREP_PER = 4, GREP_TILE = GREP_THREADS * GREP_PER; /* texts per tile of pass 3 */
constexpr uint32_t GREP_WAVES = GREP_THREADS / WAVE;
constexpr uint32_t GREP_OUT_TILE_DEFAULT = 16384, GREP_OUT_TILE_MIN = 256, GREP_OUT_TILE_MAX = 1u << 20; /* bytes of output */
static_assert (GREP_THREADS == REPLACE_THREADS, "replace_wave_count_le and replace_shfl_up are shared");

/* control words at the head of the passes' scratch, cleared in front of every call */
struct GrepCtl {
  BatchCtl batch;           /* .bad: offsets[] break the contract (batch_index_kernel) */
  unsigned long long need;  /* largest record count of a window so far */
  unsigned long long total; /* sum of all hits (pass 3, COUNT) */
};

struct GrepK {
  /* pass 2 */
  const ACMRecord *rec;            /* the window's records, in no order */
  uint64_t capacity;               /* of `rec` */
  const unsigned long long *n_dev; /* the window's record count (device) */
  uint64_t read_begin;             /* the window's positions are relative to this symbol of the buffer */
  const uint64_t *offsets;         /* [n_texts + 1] */
  uint64_t n_texts, n_symbols;
  const uint32_t *index;           /* [n_blocks]: text of position b << BATCH_BLOCK_LOG2 */
  unsigned long long *hits;        /* [n_texts] scratch counters */
  /* pass 3 */
  uint32_t flags;                  /* ACM_GREP_* */
  uint32_t *tile_kept;             /* [n_tiles + 1] kept texts per tile (the last entry stays 0) */
  const uint32_t *tile_kept_begin; /* [n_tiles + 1] their exclusive prefix sum: [n_tiles] = n_kept */
  unsigned long long *tile_sym;    /* [n_tiles + 1] symbols of the kept texts per tile */
  const unsigned long long *tile_sym_begin; /* [n_tiles + 1] their exclusive prefix sum: [n_tiles] = out_symbols */
  uint64_t n_tiles;                /* tiles of n_texts texts */
  uint32_t *kept;                  /* [n_texts] scratch: the kept texts' ids */
  unsigned long long *kept_off;    /* [n_texts + 1] scratch: their offsets in the output */
  unsigned long long *d_hits;      /* the caller's, each may be NULL */
  uint32_t *d_kept;
  unsigned long long *d_out_offsets;
  unsigned long long *d_n_kept, *d_total, *d_need, *d_out_symbols; /* (d_out_symbols may be NULL) */
  /* pass 4 */
  const unsigned char *text;
  unsigned char *out;
  uint64_t out_capacity;
  uint32_t sb;                     /* bytes per symbol of the caller's text */
  uint32_t tile_words;             /* 16-byte words per tile of pass 4 */
  GrepCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* the call reports nothing: bad offsets, or a window that found more records than there is room for */
__device__ __forceinline__ bool
grep_stopped (const GrepK &K) {
  return K.ctl->batch.bad != 0 || K.ctl->need > K.capacity;
}

/* the text of record r of a window read from symbol read_begin on, and whether the record counts:
 * its position through the index (batch_text_of between the index entries of its block and the
 * next), kept iff the match begins inside that text (batch_filter_kernel's test).  A position
 * outside the buffer (never expected) sets `wrong` and does not count.  Shared with
 * dev_tally_batch.h. */
__device__ __forceinline__ bool
grep_record_text (const uint4 r, uint64_t read_begin, const uint64_t *offsets, uint64_t n_texts, uint64_t n_symbols, const uint32_t *index,
                  uint32_t &t, bool &wrong) {
  const uint64_t rel = ((uint64_t)r.y << 32) | r.x;
  const uint64_t pos = rel + read_begin;
  if (rel >= n_symbols || pos >= n_symbols) { /* not a position of the buffer: reported, not counted */
    wrong = true;
    return false;
  }
  const uint64_t b = pos >> BATCH_BLOCK_LOG2;
  uint64_t lo = index[b], hi = index[b + 1];
  if (hi > n_texts - 1)
    hi = n_texts - 1;
  if (lo > hi)
    lo = hi;
  const uint64_t tt = batch_text_of (offsets, lo, hi, pos);
  t = (uint32_t)tt;
  return pos + 1 >= offsets[tt] + r.z; /* the match begins inside its text */
}

/* pass 2 */
__global__ __launch_bounds__ (GREP_THREADS) void
grep_hits_kernel (GrepK K) {
  const unsigned long long n = *K.n_dev;
  /* an earlier window of this call overflowed: the call reports nothing, only `need` still grows
   * (the value read is that of the earlier kernels; this kernel's own count is checked by itself) */
  const bool lost = K.ctl->need > K.capacity;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicMax (&K.ctl->need, n);
  if (n > K.capacity || lost || K.ctl->batch.bad) /* (uniform in the grid) */
    return;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool wrong = false;
  /* (the loop's condition is uniform in the wave: the ballots see every lane) */
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
    const uint64_t i = base + lane;
    bool keep = false;
    uint32_t t = 0;
    if (i < n)
      keep = grep_record_text (*reinterpret_cast<const uint4 *> (&K.rec[i]), K.read_begin, K.offsets, K.n_texts, K.n_symbols, K.index, t, wrong);
    const unsigned long long m = __ballot (keep);
    if (m == 0)
      continue;
    const uint32_t t0 = (uint32_t)__shfl ((int)t, __ffsll (m) - 1, WAVE);
    const unsigned long long same = __ballot (keep && t == t0);
    if (keep) {
      if (t != t0)
        atomicAdd (&K.hits[t], 1ull);
      else if ((int)lane == __ffsll (same) - 1)
        atomicAdd (&K.hits[t0], (unsigned long long)__popcll (same));
    }
  }
  if (wrong && K.error)
    *K.error = 1;
}

/* pass 3 */
template <bool WRITE>
__global__ __launch_bounds__ (GREP_THREADS) void
grep_flag_kernel (GrepK K) {
  __shared__ uint32_t wave_kept[GREP_PER * GREP_WAVES];
  __shared__ unsigned long long wave_sym[GREP_PER * GREP_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const bool stop = grep_stopped (K);
  if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long n_kept = stop ? 0ull : K.tile_kept_begin[K.n_tiles], all = stop ? 0ull : K.tile_sym_begin[K.n_tiles];
    *K.d_need = K.ctl->need;
    *K.d_n_kept = n_kept;
    *K.d_total = stop ? 0ull : K.ctl->total;
    if (K.d_out_symbols)
      *K.d_out_symbols = all;
    if (!stop) {
      K.kept_off[n_kept] = all;
      if (K.d_out_offsets)
        K.d_out_offsets[n_kept] = all;
    }
  }
  if (WRITE && stop) /* every other output stays as it was */
    return;
  const bool invert = (K.flags & 1u) != 0;
  unsigned long long hit_sum = 0;
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * GREP_TILE;
    if (stop || tile == K.n_tiles) { /* (uniform in the block) nothing here: the prefix sums still read the entry */
      if (!WRITE && threadIdx.x == 0) {
        K.tile_kept[tile] = 0;
        K.tile_sym[tile] = 0;
      }
      continue;
    }
    bool keep[GREP_PER];
    uint32_t rank[GREP_PER];
    unsigned long long front[GREP_PER]; /* symbols of the kept texts of the wave in front of this lane's */
#pragma unroll
    for (int q = 0; q < (int)GREP_PER; q++) {
      const uint64_t t = base + (uint64_t)q * GREP_THREADS + threadIdx.x;
      keep[q] = false;
      unsigned long long len = 0;
      if (t < K.n_texts) {
        const unsigned long long h = K.hits[t];
        hit_sum += h;
        keep[q] = (h > 0) != invert;
        if (keep[q])
          len = K.offsets[t + 1] - K.offsets[t];
        if (WRITE && K.d_hits)
          K.d_hits[t] = h;
      }
      const unsigned long long m = __ballot (keep[q]);
      rank[q] = rank_below (m);
      unsigned long long v = len;
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long o = (unsigned long long)replace_shfl_up ((long long)v, d);
        if ((int)lane >= d)
          v += o;
      }
      front[q] = v - len;
      if (lane == WAVE - 1) {
        wave_kept[q * GREP_WAVES + wave] = (uint32_t)__popcll (m);
        wave_sym[q * GREP_WAVES + wave] = v;
      }
    }
    __syncthreads ();
    if (!WRITE) {
      if (threadIdx.x == 0) {
        uint32_t k = 0;
        unsigned long long s = 0;
#pragma unroll
        for (int j = 0; j < (int)(GREP_PER * GREP_WAVES); j++) {
          k += wave_kept[j];
          s += wave_sym[j];
        }
        K.tile_kept[tile] = k;
        K.tile_sym[tile] = s;
      }
    } else {
      /* index order within the tile is (q, wave, lane): what is kept in front of this lane's text */
      const uint64_t begin_k = K.tile_kept_begin[tile];
      const unsigned long long begin_s = K.tile_sym_begin[tile];
#pragma unroll
      for (int q = 0; q < (int)GREP_PER; q++) {
        uint32_t before_k = 0;
        unsigned long long before_s = 0;
#pragma unroll
        for (int j = 0; j < (int)(GREP_PER * GREP_WAVES); j++) {
          const bool in_front = j < q * (int)GREP_WAVES + (int)wave;
          before_k += in_front ? wave_kept[j] : 0u;
          before_s += in_front ? wave_sym[j] : 0ull;
        }
        if (keep[q]) {
          const uint64_t at = begin_k + before_k + rank[q];
          const uint32_t t = (uint32_t)(base + (uint64_t)q * GREP_THREADS + threadIdx.x);
          const unsigned long long off = begin_s + before_s + front[q];
          K.kept[at] = t;
          K.kept_off[at] = off;
          if (K.d_kept)
            K.d_kept[at] = t;
          if (K.d_out_offsets)
            K.d_out_offsets[at] = off;
        }
      }
    }
    __syncthreads (); /* (the next tile's counts go into the same words) */
  }
  if (!WRITE) { /* one add per wave into the call's total */
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1)
      hit_sum += ((unsigned long long)__shfl_xor ((uint32_t)(hit_sum >> 32), d, WAVE) << 32) | __shfl_xor ((uint32_t)hit_sum, d, WAVE);
    if (lane == 0 && hit_sum)
      atomicAdd (&K.ctl->total, hit_sum);
  }
}

/* pass 4 */
__global__ __launch_bounds__ (GREP_THREADS) void
grep_gather_kernel (GrepK K) {
  __shared__ long long s_first, s_last;
  if (grep_stopped (K))
    return;
  const unsigned long long out_symbols = K.tile_sym_begin[K.n_tiles];
  if (out_symbols == 0 || out_symbols > K.out_capacity) /* no room: the caller sees the need, nothing is written */
    return;
  const uint64_t n_kept = K.tile_kept_begin[K.n_tiles];
  const long long sb = K.sb;
  const long long total = (long long)out_symbols * sb;
  const long long *const koff = reinterpret_cast<const long long *> (K.kept_off); /* [n_kept + 1], never decreasing, [n_kept] = out_symbols */
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t> (K.out) & 15);
  uint4 *const grid = reinterpret_cast<uint4 *> (K.out - mis); /* word w = out[16 w - mis, 16 w - mis + 16) */
  const long long n_words = (total + mis + 15) / 16, TW = K.tile_words;
  const long long tiles = (n_words + TW - 1) / TW;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long w0 = tile * TW, w1 = w0 + TW < n_words ? w0 + TW : n_words;
    const long long lo_b = w0 * 16 > mis ? w0 * 16 - mis : 0; /* the tile's bytes of the output */
    const long long hi_b = w1 * 16 - mis < total ? w1 * 16 - mis : total;
    if (threadIdx.x < WAVE) { /* the kept texts that hold the tile's first and last symbol: koff[0] = 0 and koff[n_kept] lies
                               * behind every symbol, so both counts lie in [1, n_kept]; of kept texts without a symbol
                               * (INVERT keeps the empty ones) that begin at the same place the last one counts */
      const uint64_t c = replace_wave_count_le (koff, n_kept + 1, lo_b / sb);
      const uint64_t c_end = replace_wave_count_le (koff, n_kept + 1, (hi_b - 1) / sb);
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
      long long l = jf, h = jl; /* the last kept text that begins at or in front of symbol s: koff[jf] <= s */
      while (l < h) {
        const long long mid = (l + h + 1) / 2;
        if (koff[mid] <= s)
          l = mid;
        else
          h = mid - 1;
      }
      long long j = l, os = koff[j] * sb, oe = koff[j + 1] * sb;
      const unsigned char *src = K.text + K.offsets[K.kept[j]] * (uint64_t)sb;
      const bool whole = b0 >= 0 && b0 + 16 <= total;
      if (whole && b0 + 16 <= oe) { /* inside one text */
        grid[w] = replace_load16 (src + (b0 - os));
      } else { /* across a boundary, or the first or last word of a buffer off the grid: byte by byte */
        uint32_t v[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int t = 0; t < 16; t++) {
          const long long b = b0 + t;
          if (b < 0 || b >= total)
            continue;
          if (b >= oe) {
            do { /* (b < total = koff[n_kept] * sb: the walk ends at a kept text in front of n_kept) */
              j++;
              os = oe;
              oe = koff[j + 1] * sb;
            } while (b >= oe);
            src = K.text + K.offsets[K.kept[j]] * (uint64_t)sb;
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
