/* dev_words.h -- whole-word matches: WORDS of a record set (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * WORDS is a function of the records and of the two symbols next to each match, so it is one
 * stable compaction of a record set in ANY order (no scan kernel touched): a record is kept iff the
 * symbol in front of its first symbol and / or the symbol behind its last one is no word symbol, or
 * lies outside the record's text.  The word set is up to 16 inclusive ranges of the caller's
 * symbols, which arrive as kernel arguments; the symbols are the caller's own, bit for bit.
 * Tiles of K.tile records (a multiple of 64), blocks stride over the tiles, a wave takes 64
 * consecutive records at a time.  Behind offsets_check_kernel (dev_batch.h; offsets[] given: the batch contract,
 * first 0, last n_symbols, non-decreasing, checked in a launch of its own so that no address is
 * formed from an offset the check has not seen), two passes with a prefix sum between them
 * (hipCUB, 64-bit, over n_tiles + 1 entries):
 *   1. words_mark_kernel: a lane takes one record, validates it (a position outside [pos_base,
 *      pos_base + n_symbols), a start below pos_base, a length of 0: dropped, the plan's error flag
 *      raised, nothing loaded), finds its text by a bisection of offsets[], drops it silently when it
 *      ends behind its text, and loads at most the two neighbour symbols -- naturally aligned loads of
 *      one symbol, never of a symbol outside the record's text.  __ballot gives the wave's keep mask,
 *      which goes to mask[record / 64]; the popcounts are summed per wave and reduced through LDS
 *      into tile_count[tile].
 *   2. words_write_kernel: reads the masks back (no second gather of the text, no second
 *      bisection: DESIGN.md says why split recomputes and this does not), ranks inside the block --
 *      the waves' popcounts through LDS, the popcount of the mask below the lane -- and stores
 *      out[tile_begin + rank] = record as one 16-byte store.  One lane writes *d_count.
 * Every output slot is written once, by one lane; no atomics.  Tiles are consecutive runs of the
 * input and ranks follow the record index: the compaction is stable.  Launch geometry never depends
 * on what the records or the text hold: capped grids, grid-stride loops over the tiles. */
constexpr uint32_t WORDS_THREADS = 256, WORDS_WAVES = WORDS_THREADS / WAVE;
constexpr uint32_t WORDS_TILE_DEFAULT = 4096, WORDS_TILE_MIN = 64, WORDS_TILE_MAX = 1u << 20; /* records */

/* control words at the head of the pass's scratch, cleared in front of every call */
struct WordsCtl {
  unsigned long long n;     /* records the passes work on (0 after an overflow and under bad offsets) */
  unsigned long long n_raw; /* the count as it came in: what *d_count keeps after an overflow */
  unsigned int bad;         /* offsets[] break the batch contract: nothing is kept */
  unsigned int pad[3];
};

struct WordsK {
  const unsigned char *text;           /* the caller's pointer: any multiple of sb */
  uint64_t n_symbols, pos_base;
  const uint64_t *offsets;             /* [n_texts + 1], NULL: one text */
  uint64_t n_texts;
  unsigned long long lo[ACM_WORDS_MAX_RANGES], hi[ACM_WORDS_MAX_RANGES]; /* the word set, inclusive */
  uint32_t n_ranges, flags;            /* ACM_WORDS_LEFT | ACM_WORDS_RIGHT */
  const ACMRecord *in;                 /* any order */
  uint64_t capacity;                   /* of `in` and `out`; the count itself when n_dev is NULL */
  const unsigned long long *n_dev;     /* the record count (device), or NULL */
  uint32_t tile;                       /* records per tile, a multiple of WAVE */
  uint64_t n_tiles;                    /* tiles of `capacity` records */
  unsigned long long *mask;            /* [(capacity + 63) / 64] keep bits of 64 consecutive records */
  unsigned long long *tile_count;      /* [n_tiles + 1] kept records per tile (the last entry stays 0) */
  const unsigned long long *tile_begin; /* [n_tiles + 1] their exclusive prefix sum: [n_tiles] = all kept records */
  ACMRecord *out;
  unsigned long long *d_count;         /* may be n_dev: read in pass 1 only, written in pass 2 only */
  WordsCtl *ctl;
  unsigned int *error;                 /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* symbol i of the text, i in [0, n_symbols): one naturally aligned load */
template <int SB>
__device__ __forceinline__ unsigned long long
words_symbol (const WordsK &K, uint64_t i) {
  const unsigned char *p = K.text + i * SB;
  if (SB == 1)
    return *p;
  if (SB == 2)
    return *reinterpret_cast<const unsigned short *> (p);
  if (SB == 4)
    return *reinterpret_cast<const unsigned int *> (p);
  return *reinterpret_cast<const unsigned long long *> (p);
}

__device__ __forceinline__ bool
words_is_word (const WordsK &K, unsigned long long x) {
  bool in = false;
  for (uint32_t j = 0; j < K.n_ranges; j++)
    in = in || (x >= K.lo[j] && x <= K.hi[j]);
  return in;
}

/* WORDS of one record; `bad` says that it breaks the contract */
template <int SB>
__device__ __forceinline__ bool
words_keep (const WordsK &K, const uint4 r, bool &bad) {
  const uint64_t pos = ((uint64_t)r.y << 32) | r.x;
  if (record_breaks_contract (pos, r.z, K.pos_base, K.n_symbols)) {
    bad = true;
    return false;
  }
  const uint64_t e = pos - K.pos_base, s = e + 1 - r.z; /* 0 <= s <= e < n_symbols */
  uint64_t t_lo = 0, t_hi = K.n_symbols;                /* the record's text: [t_lo, t_hi) */
  if (K.offsets) { /* (uniform; checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols) */
    const uint64_t t = batch_text_of (K.offsets, 0, K.n_texts - 1, s);
    t_lo = K.offsets[t];
    t_hi = K.offsets[t + 1];
    if (e >= t_hi) /* the match spans a cut: no match of any text */
      return false;
  }
  if ((K.flags & ACM_WORDS_LEFT) && s > t_lo && words_is_word (K, words_symbol<SB> (K, s - 1)))
    return false;
  if ((K.flags & ACM_WORDS_RIGHT) && e + 1 < t_hi && words_is_word (K, words_symbol<SB> (K, e + 1)))
    return false;
  return true;
}

/* pass 1 */
template <int SB>
__global__ __launch_bounds__ (WORDS_THREADS) void
words_mark_kernel (WordsK K) {
  __shared__ uint32_t wave_sum[WORDS_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  const uint64_t n = n_raw > K.capacity || K.ctl->bad ? 0 : n_raw; /* an overflowing scan left nothing to filter */
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    K.ctl->n = n;
    K.ctl->n_raw = n_raw;
  }
  bool bad = false;
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n || tile == K.n_tiles) { /* (uniform in the block) nothing here: the prefix sum still reads the entry */
      if (threadIdx.x == 0)
        K.tile_count[tile] = 0;
      continue;
    }
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    uint32_t count = 0;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += WORDS_THREADS) { /* (uniform in the wave) */
      const uint64_t i = i0 + lane;
      bool keep = false;
      if (i < n)
        keep = words_keep<SB> (K, *reinterpret_cast<const uint4 *> (&K.in[i]), bad);
      const unsigned long long m = __ballot (keep);
      if (lane == 0)
        K.mask[i0 / WAVE] = m;
      count += (uint32_t)__popcll (m);
    }
    if (lane == 0)
      wave_sum[wave] = count;
    __syncthreads ();
    if (threadIdx.x == 0) {
      uint32_t all = 0;
#pragma unroll
      for (int j = 0; j < (int)WORDS_WAVES; j++)
        all += wave_sum[j];
      K.tile_count[tile] = all;
    }
    __syncthreads (); /* (the next tile's sums go into the same words) */
  }
  if (bad && K.error)
    *K.error = 1;
}

/* pass 2 */
__global__ __launch_bounds__ (WORDS_THREADS) void
words_write_kernel (WordsK K) {
  __shared__ uint32_t wave_sum[WORDS_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = K.ctl->n;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_count = K.ctl->n_raw > K.capacity ? K.ctl->n_raw : K.tile_begin[K.n_tiles];
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) pass 1 wrote no mask here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    unsigned long long at = K.tile_begin[tile]; /* where the step's first kept record goes */
    for (uint64_t step = base; step < end; step += WORDS_THREADS) { /* (uniform in the block) */
      const uint64_t i0 = step + (uint64_t)wave * WAVE;
      const unsigned long long m = i0 < end ? K.mask[i0 / WAVE] : 0ull;
      if (lane == 0)
        wave_sum[wave] = (uint32_t)__popcll (m);
      __syncthreads ();
      uint32_t before = 0, all = 0;
#pragma unroll
      for (int j = 0; j < (int)WORDS_WAVES; j++) {
        before += j < (int)wave ? wave_sum[j] : 0u;
        all += wave_sum[j];
      }
      if ((m >> lane) & 1ull) /* (a bit is set only for a record below n) */
        *reinterpret_cast<uint4 *> (&K.out[at + before + rank_below (m)]) = *reinterpret_cast<const uint4 *> (&K.in[i0 + lane]);
      at += all;
      __syncthreads (); /* (the next step's popcounts go into the same words) */
    }
  }
}
