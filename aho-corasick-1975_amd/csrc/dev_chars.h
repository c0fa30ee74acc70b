/* dev_chars.h -- byte positions in code points and UTF-16 units: CHARS (include/acm_chars.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * Two counts decide everything: starts (a, b), the bytes of text[a, b) that are no continuation ((b & 0xC0) != 0x80),
 * and wides (a, b), its bytes >= 0xF0.  The RULER is their rank structure over one text, the MAP reads it per record.
 *
 * The text is read as dev_split.h reads it: the aligned 16-byte words that hold it, word w = the bytes
 * [16 w - mis, 16 w - mis + 16) of the text, mis = the text's address mod 16, the bytes outside [0, n) masked.  All
 * ruler geometry lives in that ALIGNED space (a = i + mis for byte i of the text), so that chunks and tiles begin at
 * aligned words whatever the caller's alignment: a chunk is C = 64, 128 or 256 bytes, a tile T bytes, a multiple of 256.
 * A 32-bit word is classified four bytes at a time: bit 0 of every byte of (x >> 7) & ~(x >> 6) says continuation,
 * of (x >> 7) & (x >> 6) & (x >> 5) & (x >> 4) says wide lead; the valid bytes are a 16-bit mask spread to the same
 * bit of every byte by one multiplication (the product's partial bits are all distinct: no carry); popcounts.
 *
 * chars_ruler_kernel: one read of the text.  Blocks stride over the tiles, a block walks its tile 256 words at a
 * time; the two counts of a lane's word travel packed in one register through the block-local scan (shuffles inside
 * the wave, the waves' totals through LDS: a step holds at most 4,096 of either, so the 16-bit fields never carry),
 * the steps in front in a running sum per count.  The first lane of every chunk stores the chunk's entry: the two
 * EXCLUSIVE in-tile counts in front of it.  One lane stores the tile's two totals; hipCUB's exclusive sum (64-bit,
 * n_tiles + 1 entries, each count on its own) turns them into the tile prefixes inside the ruler, whose last entry is
 * the whole text's count.  No second pass over the text, no atomic.
 * The ruler: a CharsHead (what it was built over and where its arrays lie), starts[n_tiles + 1], wides[n_tiles + 1],
 * entry[chunks] (8 bytes a chunk: n / 16 bytes at C = 128).
 *
 * rank (i) = tile prefix + chunk entry + the masked popcount of the at most C - 1 bytes in front of i inside its chunk
 * (aligned 16-byte loads of words that hold a byte of the range, so nothing outside the text's words is touched);
 * rank (n) is the last tile prefix, which answers it also when n ends a chunk and a tile.
 * chars_records_kernel, chars_positions_kernel: a lane per record or position, grid-stride, stores coalesced over the
 * index.  char_start = rank (s) - rank (lo), lo by batch_text_of; char_len is counted directly over [s, e + 1) when
 * both ends lie in one chunk, from rank (e + 1) otherwise; the edge bits are single byte loads of text[s] and
 * text[e + 1], skipped at lo, at hi and at the end of the buffer.  A record that breaks the contract, or any record
 * under a ruler that was not built over this text, loads nothing, gets zeros and ACM_CHARS_EDGE_BAD and raises the
 * plan's flag.  offsets[] are checked by offsets_check_kernel in a launch of its own in front. */
constexpr uint32_t CHARS_THREADS = 256, CHARS_WAVES = CHARS_THREADS / WAVE;
constexpr uint32_t CHARS_TILE_DEFAULT = 65536, CHARS_TILE_MIN = 256, CHARS_TILE_MAX = 1u << 20; /* bytes of text */
constexpr uint32_t CHARS_CHUNK_DEFAULT = 128, CHARS_CHUNK_MIN = 64, CHARS_CHUNK_MAX = 256;        /* bytes of text */
constexpr uint32_t CHARS_MAGIC = 0x52414843u;

/* the head of a ruler: what it was built over, and where its arrays lie (bytes from the head) */
struct CharsHead {
  uint32_t magic, chunk_log2, mis, tile_words;
  unsigned long long n_symbols, n_tiles, starts_at, wides_at, entry_at, pad;
};
static_assert (sizeof (CharsHead) == 64, "the arrays behind the head stay on 16 bytes");

struct CharsRulerK {
  const unsigned char *text; /* the caller's pointer: any alignment */
  CharsHead H;               /* written to *head by the pass */
  uint64_t n_words;          /* aligned 16-byte words that hold the text */
  unsigned long long *tile_starts, *tile_wides; /* [n_tiles + 1] the tiles' totals (the last entry stays 0): the sums' input */
  uint2 *entry;              /* [chunks] (starts, wides) in front of the chunk inside its tile */
  CharsHead *head;
};

/* control words at the head of a map's scratch, cleared in front of every call */
struct CharsCtl {
  unsigned int bad; /* offsets[] break the batch contract: nothing is written */
  unsigned int pad[3];
};

struct CharsMapK {
  const unsigned char *text;
  uint64_t n_symbols, pos_base;
  uint32_t mis, utf16;
  const uint64_t *offsets; /* [n_texts + 1], NULL: one text */
  uint64_t n_texts;
  const unsigned char *ruler;
  const ACMRecord *in;             /* records: any order */
  const unsigned long long *pos;   /* positions */
  uint64_t capacity;               /* of the input and the outputs; the count itself when n_dev is NULL */
  const unsigned long long *n_dev; /* the count (device), or NULL */
  unsigned long long *char_start;  /* each of the three may be NULL */
  uint32_t *char_len;
  unsigned char *edge;
  unsigned long long *out;         /* positions */
  CharsCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* the same bit of every byte of a 32-bit word from four bits side by side */
__device__ __forceinline__ uint32_t
chars_spread4 (uint32_t b4) {
  return (b4 * 0x00204081u) & 0x01010101u;
}

/* starts | wides << 16 of the bytes [lo, hi) of one 16-byte word, 0 <= lo <= hi <= 16 */
__device__ __forceinline__ uint32_t
chars_word_counts (const uint4 v, uint32_t lo, uint32_t hi) {
  const uint32_t valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
  const uint32_t x[4] = { v.x, v.y, v.z, v.w };
  uint32_t s = 0, wd = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t ok = chars_spread4 ((valid >> (4 * q)) & 0xFu);
    const uint32_t cont = (x[q] >> 7) & ~(x[q] >> 6) & 0x01010101u;
    const uint32_t wide = (x[q] >> 7) & (x[q] >> 6) & (x[q] >> 5) & (x[q] >> 4) & 0x01010101u;
    s += (uint32_t)__popc (ok & ~cont);
    wd += (uint32_t)__popc (ok & wide);
  }
  return s | (wd << 16);
}

/* the aligned word w of a text that lies `mis` bytes behind a 16-byte boundary */
__device__ __forceinline__ uint4
chars_load_word (const unsigned char *text, uint32_t mis, uint64_t w) {
  return *reinterpret_cast<const uint4 *> (text + ((long long)(w * 16) - (long long)mis));
}

__global__ __launch_bounds__ (CHARS_THREADS) void
chars_ruler_kernel (CharsRulerK K) {
  __shared__ uint32_t wave_sum[CHARS_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.head = K.H;
  const uint32_t mis = K.H.mis, word_shift = K.H.chunk_log2 - 4, in_chunk = (1u << word_shift) - 1u;
  const long long total = (long long)K.H.n_symbols;
  for (uint64_t tile = blockIdx.x; tile <= K.H.n_tiles; tile += gridDim.x) {
    if (tile == K.H.n_tiles) { /* (uniform in the block) the prefix sums read the entry */
      if (threadIdx.x == 0) {
        K.tile_starts[tile] = 0;
        K.tile_wides[tile] = 0;
      }
      continue;
    }
    const uint64_t w0 = tile * K.H.tile_words, w1 = w0 + K.H.tile_words < K.n_words ? w0 + K.H.tile_words : K.n_words;
    uint32_t run_s = 0, run_w = 0; /* the counts of the steps in front (at most 2^20 each) */
    for (uint64_t base = w0; base < w1; base += CHARS_THREADS) { /* (uniform in the block) */
      const uint64_t w = base + threadIdx.x;
      uint32_t mine = 0;
      if (w < w1) {
        const long long b0 = (long long)(w * 16) - (long long)mis; /* the word's first byte, as a byte of the text */
        const uint32_t lo = b0 < 0 ? (uint32_t)(-b0) : 0u;
        const uint32_t hi = total - b0 >= 16 ? 16u : (uint32_t)(total - b0);
        mine = chars_word_counts (chars_load_word (K.text, mis, w), lo, hi);
      }
      uint32_t incl = mine; /* both counts of the wave's lanes up to this one: at most 1,024 a field */
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
      for (int j = 0; j < (int)CHARS_WAVES; j++) {
        before += j < (int)wave ? wave_sum[j] : 0u;
        all += wave_sum[j];
      }
      if (w < w1 && (w & in_chunk) == 0) { /* the chunk's first word */
        const uint32_t excl = before + incl - mine;
        K.entry[w >> word_shift] = make_uint2 (run_s + (excl & 0xFFFFu), run_w + (excl >> 16));
      }
      run_s += all & 0xFFFFu;
      run_w += all >> 16;
      __syncthreads (); /* (the next step's totals go into the same words) */
    }
    if (threadIdx.x == 0) {
      K.tile_starts[tile] = run_s;
      K.tile_wides[tile] = run_w;
    }
  }
}

/* a ruler as the maps read it */
struct CharsRuler {
  const long long *starts, *wides;
  const uint2 *entry;
  uint32_t chunk_log2, tile_words;
  uint64_t n_tiles;
  bool ok; /* built over this text */
};

__device__ __forceinline__ CharsRuler
chars_ruler_open (const CharsMapK &K) {
  const CharsHead *h = reinterpret_cast<const CharsHead *> (K.ruler);
  CharsRuler R;
  R.ok = h->magic == CHARS_MAGIC && h->n_symbols == K.n_symbols && h->mis == K.mis;
  R.starts = reinterpret_cast<const long long *> (K.ruler + h->starts_at);
  R.wides = reinterpret_cast<const long long *> (K.ruler + h->wides_at);
  R.entry = reinterpret_cast<const uint2 *> (K.ruler + h->entry_at);
  R.chunk_log2 = h->chunk_log2;
  R.tile_words = h->tile_words;
  R.n_tiles = h->n_tiles;
  return R;
}

/* count of the aligned-space bytes [a0, a1), mis <= a0 <= a1 <= n + mis, fewer than 2^16 of them: every word loaded
 * holds a byte of the range */
__device__ __forceinline__ unsigned long long
chars_range_count (const CharsMapK &K, uint64_t a0, uint64_t a1) {
  uint32_t c = 0;
  if (a0 < a1)
    for (uint64_t w = a0 >> 4; (w << 4) < a1; w++) {
      const uint64_t b = w << 4;
      const uint32_t lo = a0 > b ? (uint32_t)(a0 - b) : 0u;
      const uint32_t hi = a1 - b >= 16 ? 16u : (uint32_t)(a1 - b);
      c += chars_word_counts (chars_load_word (K.text, K.mis, w), lo, hi);
    }
  return (c & 0xFFFFu) + (K.utf16 ? c >> 16 : 0u);
}

/* count (0, i), 0 <= i <= n */
__device__ __forceinline__ unsigned long long
chars_rank (const CharsMapK &K, const CharsRuler &R, uint64_t i) {
  if (i >= K.n_symbols)
    return (unsigned long long)R.starts[R.n_tiles] + (K.utf16 ? (unsigned long long)R.wides[R.n_tiles] : 0ull);
  const uint64_t a = i + K.mis, chunk = a >> R.chunk_log2, tile = (a >> 4) / R.tile_words;
  const uint2 e = R.entry[chunk];
  const uint64_t c0 = chunk << R.chunk_log2;
  unsigned long long r = (unsigned long long)R.starts[tile] + e.x;
  if (K.utf16)
    r += (unsigned long long)R.wides[tile] + e.y;
  return r + chars_range_count (K, c0 < K.mis ? K.mis : c0, a);
}

__device__ __forceinline__ bool
chars_is_continuation (const CharsMapK &K, uint64_t i) {
  return (K.text[i] & 0xC0) == 0x80;
}

/* the items a map works on: none after an overflow and under bad offsets */
__device__ __forceinline__ uint64_t
chars_n (const CharsMapK &K) {
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  return n_raw > K.capacity || K.ctl->bad ? 0 : n_raw;
}

__global__ __launch_bounds__ (CHARS_THREADS) void
chars_records_kernel (CharsMapK K) {
  const uint64_t n = chars_n (K), stride = (uint64_t)gridDim.x * CHARS_THREADS;
  const CharsRuler R = chars_ruler_open (K);
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * CHARS_THREADS + threadIdx.x; i < n; i += stride) {
    const uint4 r = *reinterpret_cast<const uint4 *> (&K.in[i]);
    const uint64_t pos = ((uint64_t)r.y << 32) | r.x;
    unsigned long long start = 0;
    uint32_t len = 0, edge = ACM_CHARS_EDGE_BAD;
    if (!R.ok || record_breaks_contract (pos, r.z, K.pos_base, K.n_symbols))
      bad = true;
    else {
      const uint64_t e = pos - K.pos_base, s = e + 1 - r.z; /* 0 <= s <= e < n_symbols */
      uint64_t lo = 0, hi = K.n_symbols;                    /* the text of s: [lo, hi) */
      if (K.offsets) { /* (uniform; checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols) */
        const uint64_t t = batch_text_of (K.offsets, 0, K.n_texts - 1, s);
        lo = K.offsets[t];
        hi = K.offsets[t + 1];
      }
      const unsigned long long rank_s = chars_rank (K, R, s);
      start = rank_s - chars_rank (K, R, lo);
      const uint64_t a0 = s + K.mis, a1 = e + 1 + K.mis;
      len = (uint32_t)((a0 >> R.chunk_log2) == ((a1 - 1) >> R.chunk_log2) ? chars_range_count (K, a0, a1) : chars_rank (K, R, e + 1) - rank_s);
      edge = (s != lo && chars_is_continuation (K, s) ? ACM_CHARS_EDGE_START : 0u) |
             (e + 1 != hi && e + 1 < K.n_symbols && chars_is_continuation (K, e + 1) ? ACM_CHARS_EDGE_END : 0u);
    }
    if (K.char_start)
      K.char_start[i] = start;
    if (K.char_len)
      K.char_len[i] = len;
    if (K.edge)
      K.edge[i] = (unsigned char)edge;
  }
  if (bad && K.error)
    *K.error = 1;
}

__global__ __launch_bounds__ (CHARS_THREADS) void
chars_positions_kernel (CharsMapK K) {
  const uint64_t n = chars_n (K), stride = (uint64_t)gridDim.x * CHARS_THREADS;
  const CharsRuler R = chars_ruler_open (K);
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * CHARS_THREADS + threadIdx.x; i < n; i += stride) {
    const uint64_t p = K.pos[i];
    unsigned long long out = 0;
    if (!R.ok || p > K.n_symbols)
      bad = true;
    else {
      const uint64_t lo = K.offsets ? K.offsets[batch_text_of (K.offsets, 0, K.n_texts - 1, p)] : 0;
      out = chars_rank (K, R, p) - chars_rank (K, R, lo);
    }
    K.out[i] = out;
  }
  if (bad && K.error)
    *K.error = 1;
}
