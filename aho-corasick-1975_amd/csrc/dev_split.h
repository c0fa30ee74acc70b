/* dev_split.h -- a buffer cut into texts at delimiter symbols: the offsets[] every batch call takes
 * (include/acm_gpu.h, SPLIT).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The text is read as the aligned 16-byte words that hold it: word w is the bytes
 * [16 w - mis, 16 w - mis + 16) of the text, mis = the text's address mod 16, so that every load is
 * one aligned uint4 whatever the caller's alignment; the symbols of the first and the last word that
 * lie outside [0, n) are masked and never count.  A word gives one bit per symbol (16 / sb bits):
 *   delimiter bits: the symbol equals one of the up to 16 delimiters, which arrive as kernel
 *     arguments.  Bytes and 2-byte symbols are compared four and two at a time inside a 32-bit word
 *     (x ^ pattern has a zero byte exactly where ((y & 0x7F..) + 0x7F..) | y has no high bit: no carry
 *     crosses a symbol, so the test is exact), about five operations per delimiter and 32-bit word;
 *   cut bits: EVERY: the delimiter bits.  RUNS: a delimiter whose NEXT symbol is none (or lies
 *     outside the buffer); the next symbol is a shift inside the word, the next lane's first bit at
 *     the word's last symbol (a shuffle), and one extra load of the next word for the last lane of a
 *     wave and the last word of a tile.  Both: the bit of symbol n - 1, the forced cut.
 * Tiles of K.tile_words words, blocks stride over the tiles, a block walks its tile 256 words at a
 * time.  Two passes, a prefix sum between (hipCUB, 64-bit, over n_tiles + 1 entries):
 *   1. split_count_kernel: popcount of the cut bits, summed per lane, reduced per block (shuffles,
 *      then the waves' sums through LDS) into tile_count[tile].
 *   2. split_write_kernel: re-reads the text and recomputes the bits (2.0 passes of traffic; no
 *      bitmask is kept: DESIGN.md says why), ranks them inside the block -- a shuffle scan of the
 *      lanes' counts, the waves' totals through LDS, the steps in front in a running sum -- and
 *      stores offsets[1 + tile_begin + rank] = symbol + 1, every store guarded by index <= capacity.
 *      Tile 0 writes offsets[0] = 0; one lane writes *d_n_texts = the sum of all tiles.  Without an
 *      offsets array (count only) one block writes the count and nothing else runs.
 * Every offset is written once, by one lane; no atomics.  Launch geometry never depends on what the
 * text holds: capped grids, grid-stride loops over the tiles. */
constexpr uint32_t SPLIT_THREADS = 256, SPLIT_WAVES = SPLIT_THREADS / WAVE;
constexpr uint32_t SPLIT_TILE_DEFAULT = 16384, SPLIT_TILE_MIN = 256, SPLIT_TILE_MAX = 1u << 20; /* bytes of text */

struct SplitK {
  const unsigned char *text;           /* the caller's pointer: any multiple of sb */
  uint64_t n_symbols;
  unsigned long long delim[ACM_SPLIT_MAX_DELIMS]; /* sb < 4: the symbol repeated over 32 bits */
  uint32_t n_delims;
  uint32_t runs;                       /* ACM_SPLIT_RUNS */
  uint32_t tile_words;                 /* 16-byte words per tile */
  uint64_t n_words, n_tiles;
  unsigned long long *tile_count;      /* [n_tiles + 1] cuts per tile (the last entry stays 0) */
  const unsigned long long *tile_begin; /* [n_tiles + 1] their exclusive prefix sum: [n_tiles] = n_texts */
  unsigned long long *offsets;         /* [capacity + 1], NULL: count only */
  uint64_t capacity;
  unsigned long long *d_n_texts;
};

/* bit k: symbol k of the word equals a delimiter */
template <int SB>
__device__ __forceinline__ uint32_t
split_delim_bits (const SplitK &K, const uint4 v) {
  const uint32_t x[4] = { v.x, v.y, v.z, v.w };
  if (SB <= 2) {
    constexpr uint32_t LOW = SB == 1 ? 0x7F7F7F7Fu : 0x7FFF7FFFu;
    uint32_t none[4] = { ~0u, ~0u, ~0u, ~0u }; /* high bit of a symbol: it equals no delimiter so far */
    for (uint32_t j = 0; j < K.n_delims; j++) {
      const uint32_t pat = (uint32_t)K.delim[j];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t y = x[q] ^ pat;
        none[q] &= ((y & LOW) + LOW) | y;
      }
    }
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t z = ~none[q] & ~LOW;
      if (SB == 1) /* the bits 7, 15, 23, 31 side by side: the products' bits are all distinct, no carry */
        bits |= ((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * q);
      else
        bits |= (((z >> 15) & 1u) | ((z >> 30) & 2u)) << (2 * q);
    }
    return bits;
  }
  uint32_t bits = 0;
  for (uint32_t j = 0; j < K.n_delims; j++) {
    const uint32_t lo = (uint32_t)K.delim[j], hi = (uint32_t)(K.delim[j] >> 32);
    if (SB == 4)
      bits |= (uint32_t)(x[0] == lo) | (uint32_t)(x[1] == lo) << 1 | (uint32_t)(x[2] == lo) << 2 | (uint32_t)(x[3] == lo) << 3;
    else
      bits |= (uint32_t)(x[0] == lo && x[1] == hi) | (uint32_t)(x[2] == lo && x[3] == hi) << 1;
  }
  return bits;
}

/* the delimiter bits of word w (w < n_words), the symbols outside the buffer masked */
template <int SB>
__device__ __forceinline__ uint32_t
split_word_delims (const SplitK &K, uint64_t w, uint32_t mis, long long total) {
  constexpr int PER = 16 / SB;
  const long long b0 = (long long)(w * 16) - (long long)mis; /* the word's first byte, as a byte of the text */
  const uint32_t lo = b0 < 0 ? (uint32_t)(-b0) / SB : 0u;
  const uint32_t hi = total - b0 >= 16 ? (uint32_t)PER : (uint32_t)(total - b0) / SB;
  const uint32_t valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
  const uint4 v = *reinterpret_cast<const uint4 *> (K.text + b0);
  return split_delim_bits<SB> (K, v) & valid;
}

/* the cut bits of word w for a lane of a block that walks [.., w1) together: EVERY lane of the wave
 * calls this (the shuffle), `mine` says whether the lane has a word */
template <int SB>
__device__ __forceinline__ uint32_t
split_word_cuts (const SplitK &K, uint64_t w, uint64_t w1, bool mine, uint32_t mis, long long total) {
  constexpr int PER = 16 / SB;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t d = mine ? split_word_delims<SB> (K, w, mis, total) : 0u;
  uint32_t cut = d;
  if (K.runs) { /* (uniform in the grid) */
    uint32_t next_first = (uint32_t)__shfl_down ((int)(d & 1u), 1, WAVE);
    if (mine && (lane == WAVE - 1 || w + 1 == w1)) /* the next word is no lane's of this wave and step */
      next_first = w + 1 < K.n_words ? split_word_delims<SB> (K, w + 1, mis, total) & 1u : 0u;
    cut = d & ~((d >> 1) | (next_first << (PER - 1)));
  }
  if (mine) { /* the forced cut behind n - 1 */
    const uint64_t last = (uint64_t)(total - SB) + mis;
    if (w == last / 16)
      cut |= 1u << ((uint32_t)(last % 16) / SB);
  }
  return cut;
}

/* pass 1 */
template <int SB>
__global__ __launch_bounds__ (SPLIT_THREADS) void
split_count_kernel (SplitK K) {
  __shared__ uint32_t wave_sum[SPLIT_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t> (K.text) & 15);
  const long long total = (long long)K.n_symbols * SB;
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    if (tile == K.n_tiles) { /* (uniform in the block) the prefix sum reads the entry */
      if (threadIdx.x == 0)
        K.tile_count[tile] = 0;
      continue;
    }
    const uint64_t w0 = tile * K.tile_words, w1 = w0 + K.tile_words < K.n_words ? w0 + K.tile_words : K.n_words;
    uint32_t count = 0;
    for (uint64_t base = w0; base < w1; base += SPLIT_THREADS) {
      const uint64_t w = base + threadIdx.x;
      count += (uint32_t)__popc (split_word_cuts<SB> (K, w, w1, w < w1, mis, total));
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1)
      count += (uint32_t)__shfl_xor ((int)count, d, WAVE);
    if (lane == 0)
      wave_sum[wave] = count;
    __syncthreads ();
    if (threadIdx.x == 0) {
      uint32_t all = 0;
#pragma unroll
      for (int j = 0; j < (int)SPLIT_WAVES; j++)
        all += wave_sum[j];
      K.tile_count[tile] = all;
    }
    __syncthreads (); /* (the next tile's sums go into the same words) */
  }
}

/* pass 2 */
template <int SB>
__global__ __launch_bounds__ (SPLIT_THREADS) void
split_write_kernel (SplitK K) {
  __shared__ uint32_t wave_sum[SPLIT_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_n_texts = K.tile_begin[K.n_tiles];
  if (!K.offsets) /* count only */
    return;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t> (K.text) & 15);
  const long long total = (long long)K.n_symbols * SB;
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t w0 = tile * K.tile_words, w1 = w0 + K.tile_words < K.n_words ? w0 + K.tile_words : K.n_words;
    if (tile == 0 && threadIdx.x == 0)
      K.offsets[0] = 0;
    unsigned long long at = 1 + K.tile_begin[tile]; /* where the step's first cut goes */
    for (uint64_t base = w0; base < w1; base += SPLIT_THREADS) {
      const uint64_t w = base + threadIdx.x;
      uint32_t cut = split_word_cuts<SB> (K, w, w1, w < w1, mis, total);
      const uint32_t mine = (uint32_t)__popc (cut);
      uint32_t incl = mine; /* the cuts of the wave's lanes up to this one */
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up ((int)incl, d, WAVE);
        if ((int)lane >= d)
          incl += o;
      }
      if (lane == WAVE - 1)
        wave_sum[wave] = incl;
      __syncthreads ();
      uint32_t before = 0, all = 0;
#pragma unroll
      for (int j = 0; j < (int)SPLIT_WAVES; j++) {
        before += j < (int)wave ? wave_sum[j] : 0u;
        all += wave_sum[j];
      }
      unsigned long long index = at + before + (incl - mine);
      const long long first = ((long long)(w * 16) - (long long)mis) / SB; /* the word's symbol 0 (exact: mis is a multiple of SB) */
      while (cut) {
        const int k = __ffs ((int)cut) - 1;
        cut &= cut - 1;
        if (index <= K.capacity)
          K.offsets[index] = (unsigned long long)(first + k + 1);
        index++;
      }
      at += all;
      __syncthreads (); /* (the next step's totals go into the same words) */
    }
  }
}
