/* dev_tokens.h -- tokenising: TOKENS of a text under a selection (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The input is a selection -- records in canonical order, no two sharing a symbol: what dev_select.h
 * leaves -- its count read on the device, optionally the offsets of a batch and a table keyword ->
 * vocabulary id.  The form is TEXT-stationary: the tokens are counted and numbered where they begin
 * in the text, because two of the three kinds of unit (gap symbols, gap runs) are no records at all
 * and tok_first[] is a rank at a position.  The passes, all behind whatever made the selection, on
 * its stream:
 *   a. tokens_check_kernel: every record against the contract (inside the text, behind the record in
 *      front of it, inside ONE text -- a bisection of offsets[] --, a keyword id of the table) and
 *      offsets[] against its own (begins with 0, never decreases, ends with n_symbols).  A violation
 *      raises the plan's error flag and counts in ctl->n_bad: every later pass then writes nothing
 *      but *d_n_tokens = 0.  No address is formed from a record or an offset before this pass has
 *      seen it; the bisection stays inside offsets[0 .. n_texts] whatever the values are.
 *   b. tokens_tile_kernel<false>: the text is cut into tiles of K.tile symbols.  A block finds the
 *      records that touch its tile (and the symbol in front of it) and the offsets that fall into it
 *      -- four 64-way searches, one wave each, over the records' ends and starts and offsets[] --
 *      and marks three bitmaps in LDS: covered symbols, match starts, text starts.  From them one
 *      word-wise pass makes the token-start bits: the match starts, and by mode every uncovered
 *      symbol (SYMBOL), every uncovered symbol behind a covered one or at a text start (RUN), or no
 *      other (DROP).  Their number goes to tile_count[].
 *   c. the exclusive prefix sum over the tiles (hipcub, 64-bit): tile_begin[], the total behind them.
 *   d. tokens_tile_kernel<true>: the same bitmaps again, a prefix over their words inside the block,
 *      and then every token is stored at its rank: a match by the lane that holds its record, a gap
 *      symbol by the lane of its position (stores of neighbouring lanes lie side by side), a gap run
 *      by the lane of its bitmap word, which looks for the run's end in the covered and text-start
 *      bits behind it and, when the tile has none, takes what lies behind the tile: the next record's
 *      start, the next offset or the end of the buffer, known from the searches.  tok_first[t] is the
 *      rank at offsets[t]; the offsets at n_symbols take the total.  Every output element is written
 *      once, by one lane; no atomics on outputs.  Stores are guarded by token_capacity; when the
 *      total exceeds it no token is stored at all, tok_first[] still is.
 * RUN and DROP never read the text; SYMBOL reads single symbols of the buffer itself.
 * Launch geometry never depends on a count on the device: capped grids, grid-stride loops. */
constexpr uint32_t TOKENS_THREADS = 256, TOKENS_WAVES = TOKENS_THREADS / WAVE;
constexpr uint32_t TOKENS_TILE_DEFAULT = 8192, TOKENS_TILE_MIN = 64, TOKENS_TILE_MAX = 16384; /* symbols, multiples of 64 */
constexpr uint32_t TOKENS_WORDS_MAX = TOKENS_TILE_MAX / 32;

/* control words at the head of the passes' scratch, cleared in front of every call */
struct TokensCtl {
  unsigned int n_bad; /* records and offsets that break the contract */
  unsigned int pad[3];
};

struct TokensK {
  const ACMRecord *sel;              /* the selection, canonical order */
  uint64_t capacity;                 /* of `sel`; the count itself when n_dev is NULL */
  const unsigned long long *n_dev;   /* the record count (device), or NULL */
  const unsigned char *text;         /* SYMBOL mode only */
  uint64_t n_symbols, pos_base;
  uint32_t sb;                       /* bytes per symbol of the caller's text */
  uint32_t mode, gap_base;
  uint32_t tile;                     /* symbols per tile */
  const unsigned long long *offsets; /* [n_texts + 1], or NULL: one text */
  uint64_t n_texts;
  const uint32_t *tok_of;            /* [n_keywords], or NULL */
  uint64_t n_keywords;
  long long *tile_count;             /* [n_tiles + 1] token starts per tile, 0 behind the last */
  const long long *tile_begin;       /* [n_tiles + 1] their exclusive prefix sum: [n_tiles] = the total */
  uint64_t n_tiles;
  uint32_t *tok_id;
  unsigned long long *tok_start;
  uint32_t *tok_len;
  uint64_t token_capacity;
  unsigned long long *d_n_tokens, *tok_first;
  TokensCtl *ctl;
  unsigned int *error;               /* the plan's device-side flag (acm_gpu_plan_status) */
};

__device__ __forceinline__ bool
tokens_overflowed (const TokensK &K) {
  return K.n_dev && *K.n_dev > K.capacity;
}

__device__ __forceinline__ uint64_t
tokens_count (const TokensK &K) {
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  return n_raw > K.capacity ? 0 : n_raw;
}

/* record i relative to the text: its first symbol, its last, its keyword */
__device__ __forceinline__ void
tokens_fact (const TokensK &K, uint64_t i, uint64_t &start, uint64_t &end, uint32_t &len, uint32_t &kw) {
  const uint4 r = *reinterpret_cast<const uint4 *> (&K.sel[i]);
  end = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
  len = r.z;
  kw = r.w;
  start = end + 1 - len;
}

/* by a whole wave: how many of f (0) <= f (1) <= ... <= f (n - 1) are <= key.  64 probes a step;
 * every probe lies in [0, n) whatever the values are. */
template <typename F>
__device__ __forceinline__ uint64_t
tokens_wave_count_le (F f, uint64_t n, uint64_t key) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  uint64_t lo = 0, hi = n; /* the answer lies in [lo, hi] */
  while (hi > lo) {
    const uint64_t step = (hi - lo + WAVE - 1) / WAVE;
    const uint64_t idx = lo + (uint64_t)(lane + 1) * step - 1;
    const bool le = idx < hi && f (idx) <= key;
    const uint64_t k = (uint64_t)__popcll (__ballot (le));
    const uint64_t fail = lo + (k + 1) * step - 1; /* the first probe that was greater, if there was one */
    lo += k * step;
    hi = fail < hi ? fail : hi;
  }
  return lo;
}

/* pass a */
__global__ __launch_bounds__ (TOKENS_THREADS) void
tokens_check_kernel (TokensK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = tokens_count (K);
  uint32_t bad = 0;
  for (uint64_t i = me; i < n; i += stride) {
    const ACMRecord r = K.sel[i];
    const uint64_t pos = r.end_pos;
    if (record_breaks_contract (pos, r.length, K.pos_base, K.n_symbols)) {
      bad++;
      continue;
    }
    const uint64_t end = pos - K.pos_base, start = end + 1 - r.length;
    if (i > 0) { /* behind the record in front of it (which answers for its own range) */
      const uint64_t prev = K.sel[i - 1].end_pos;
      if (prev < K.pos_base || prev - K.pos_base >= start) {
        bad++;
        continue;
      }
    }
    if (K.tok_of && r.keyword_id >= K.n_keywords) {
      bad++;
      continue;
    }
    if (K.offsets) { /* the first offset behind the record's start lies behind its end: one text holds it */
      uint64_t lo = 0, hi = K.n_texts + 1;
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (K.offsets[mid] <= start)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo <= K.n_texts && K.offsets[lo] <= end)
        bad++;
    }
  }
  if (K.offsets)
    for (uint64_t k = me; k <= K.n_texts; k += stride) {
      const unsigned long long o = K.offsets[k];
      bad += k == 0 ? o != 0 : K.offsets[k - 1] > o;
      bad += k == K.n_texts && o != K.n_symbols;
    }
  if (bad) {
    atomicAdd (&K.ctl->n_bad, bad);
    if (K.error)
      *K.error = 1;
  }
}

/* LDS of tokens_tile_kernel: the tile's bitmaps, bit p of word w = symbol lo + 32 w + p */
struct TokensTile {
  uint32_t cov[TOKENS_WORDS_MAX];      /* covered by a record */
  uint32_t ms[TOKENS_WORDS_MAX];       /* a record begins here */
  uint32_t ts[TOKENS_WORDS_MAX];       /* a text begins here */
  uint32_t st[TOKENS_WORDS_MAX];       /* a token begins here */
  uint32_t wpre[TOKENS_WORDS_MAX + 1]; /* token starts in the words in front of word w (pass d) */
  uint32_t wave_sum[TOKENS_WAVES];
  uint32_t prev_cov;                   /* the symbol in front of the tile is covered */
  unsigned long long c0, c1, k0, k1;   /* the records [c0, c1) touch [lo - 1, hi), the offsets [k0, k1) lie in [lo, hi) */
};

/* inclusive sums over the block's threads in thread order; the block's total in `total` */
__device__ __forceinline__ uint32_t
tokens_block_scan (uint32_t v, uint32_t *wave_sum /* [TOKENS_WAVES] LDS */, uint32_t &total) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t o = __shfl_up (v, d, WAVE);
    if ((int)lane >= d)
      v += o;
  }
  if (lane == WAVE - 1)
    wave_sum[wave] = v;
  __syncthreads ();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < (int)TOKENS_WAVES; w++) {
    before += w < (int)wave ? wave_sum[w] : 0u;
    total += wave_sum[w];
  }
  __syncthreads (); /* (the next use writes the same words) */
  return v + before;
}

/* the bits [p, q) of a bitmap, 0 <= p < q <= the tile */
__device__ __forceinline__ void
tokens_set_bits (uint32_t *map, uint32_t p, uint32_t q) {
  const uint32_t wa = p >> 5, wb = (q - 1) >> 5;
  for (uint32_t w = wa; w <= wb; w++) {
    uint32_t m = ~0u;
    if (w == wa)
      m &= ~0u << (p & 31);
    if (w == wb)
      m &= ~0u >> (31 - ((q - 1) & 31));
    atomicOr (&map[w], m);
  }
}

/* the bitmaps of the tile [lo, hi) and its token-start bits: S.st is complete behind the call */
__device__ __forceinline__ void
tokens_tile_bits (const TokensK &K, TokensTile &S, uint64_t n, uint64_t lo, uint64_t hi) {
  const uint32_t words = K.tile / 32, wave = threadIdx.x / WAVE;
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
    S.cov[w] = 0;
    S.ms[w] = 0;
    S.ts[w] = 0;
  }
  if (threadIdx.x == 0)
    S.prev_cov = 0;
  const uint64_t front = lo ? lo - 1 : 0; /* the first symbol whose cover the tile asks for */
  auto rec_end = [&] (uint64_t i) { return (uint64_t)K.sel[i].end_pos - K.pos_base; };
  auto rec_start = [&] (uint64_t i) { return (uint64_t)K.sel[i].end_pos - K.pos_base + 1 - K.sel[i].length; };
  auto offset = [&] (uint64_t i) { return (uint64_t)K.offsets[i]; };
  unsigned long long found = 0; /* (uniform in the wave) */
  if (wave == 0)
    found = front ? tokens_wave_count_le (rec_end, n, front - 1) : 0;
  else if (wave == 1)
    found = tokens_wave_count_le (rec_start, n, hi - 1);
  else if (wave == 2)
    found = K.offsets && lo ? tokens_wave_count_le (offset, K.n_texts + 1, lo - 1) : 0;
  else
    found = K.offsets ? tokens_wave_count_le (offset, K.n_texts + 1, hi - 1) : 0;
  if ((threadIdx.x & (WAVE - 1)) == 0)
    (wave == 0 ? S.c0 : wave == 1 ? S.c1 : wave == 2 ? S.k0 : S.k1) = found;
  __syncthreads ();
  const uint64_t c0 = S.c0, c1 = S.c1, k0 = S.k0, k1 = S.k1;
  for (uint64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x) {
    uint64_t s, e;
    uint32_t len, kw;
    tokens_fact (K, j, s, e, len, kw);
    if (lo && s < lo && e >= lo - 1)
      S.prev_cov = 1;
    const uint64_t a = s > lo ? s : lo, b = e + 1 < hi ? e + 1 : hi;
    if (a < b)
      tokens_set_bits (S.cov, (uint32_t)(a - lo), (uint32_t)(b - lo));
    if (s >= lo && s < hi)
      atomicOr (&S.ms[(s - lo) >> 5], 1u << ((s - lo) & 31));
  }
  for (uint64_t k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
    const uint64_t o = K.offsets[k];
    if (o >= lo && o < hi)
      atomicOr (&S.ts[(o - lo) >> 5], 1u << ((o - lo) & 31));
  }
  __syncthreads ();
  const uint32_t len = (uint32_t)(hi - lo);
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
    const uint32_t valid = w * 32 >= len ? 0u : len - w * 32 >= 32 ? ~0u : (1u << (len - w * 32)) - 1;
    const uint32_t unc = ~S.cov[w] & valid;
    uint32_t gap = 0;
    if (K.mode == ACM_TOKENS_GAP_SYMBOL)
      gap = unc;
    else if (K.mode == ACM_TOKENS_GAP_RUN) { /* behind a covered symbol, at a text start, at the buffer's first symbol */
      const uint32_t carry = w ? S.cov[w - 1] >> 31 : lo == 0 ? 1u : S.prev_cov;
      gap = unc & ((S.cov[w] << 1) | carry | S.ts[w]);
    }
    S.st[w] = S.ms[w] | gap;
  }
  __syncthreads ();
}

/* passes b (WRITE false) and d (WRITE true) */
template <bool WRITE>
__global__ __launch_bounds__ (TOKENS_THREADS) void
tokens_tile_kernel (TokensK K) {
  __shared__ TokensTile S;
  const bool stop = K.ctl->n_bad != 0 || tokens_overflowed (K);
  const uint64_t n = tokens_count (K);
  const uint32_t words = K.tile / 32, per = (words + TOKENS_THREADS - 1) / TOKENS_THREADS;
  unsigned long long total = 0;
  bool store = false;
  if (WRITE) {
    total = stop ? 0ull : (unsigned long long)K.tile_begin[K.n_tiles];
    if (blockIdx.x == 0 && threadIdx.x == 0)
      *K.d_n_tokens = total;
    store = K.tok_id != nullptr && total <= K.token_capacity;
    if (stop || (!store && !K.tok_first))
      return;
  }
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles + (WRITE ? 0 : 1); tile += gridDim.x) {
    if (!WRITE && (stop || tile == K.n_tiles)) { /* (uniform in the block; the prefix sum reads every entry) */
      if (threadIdx.x == 0)
        K.tile_count[tile] = 0;
      continue;
    }
    const uint64_t lo = tile * K.tile, hi = lo + K.tile < K.n_symbols ? lo + K.tile : K.n_symbols;
    tokens_tile_bits (K, S, n, lo, hi);
    uint32_t mine = 0;
    const uint32_t w_first = threadIdx.x * per;
    for (uint32_t q = 0; q < per; q++)
      if (w_first + q < words)
        mine += __popc (S.st[w_first + q]);
    uint32_t all;
    uint32_t at = tokens_block_scan (mine, S.wave_sum, all) - mine;
    if (!WRITE) {
      if (threadIdx.x == 0)
        K.tile_count[tile] = all;
      continue; /* (tokens_block_scan ends with a barrier: the next tile may clear the bitmaps) */
    }
    for (uint32_t q = 0; q < per; q++)
      if (w_first + q < words) {
        S.wpre[w_first + q] = at;
        at += __popc (S.st[w_first + q]);
      }
    __syncthreads ();
    const unsigned long long begin = (unsigned long long)K.tile_begin[tile];
    auto rank = [&] (uint32_t p) { /* tokens that begin in front of symbol lo + p */
      return begin + S.wpre[p >> 5] + __popc (S.st[p >> 5] & ((1u << (p & 31)) - 1));
    };
    const uint64_t c0 = S.c0, c1 = S.c1, k0 = S.k0, k1 = S.k1;
    if (K.tok_first)
      for (uint64_t k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
        const uint64_t o = K.offsets[k];
        if (o >= lo && o < hi)
          K.tok_first[k] = rank ((uint32_t)(o - lo));
      }
    if (store) {
      /* the matches that begin in the tile */
      for (uint64_t j = c0 + threadIdx.x; j < c1; j += blockDim.x) {
        uint64_t s, e;
        uint32_t len, kw;
        tokens_fact (K, j, s, e, len, kw);
        if (s < lo || s >= hi)
          continue;
        const unsigned long long r = rank ((uint32_t)(s - lo));
        if (r < K.token_capacity) {
          K.tok_id[r] = K.tok_of ? K.tok_of[kw] : kw;
          if (K.tok_start)
            K.tok_start[r] = s + K.pos_base;
          if (K.tok_len)
            K.tok_len[r] = len;
        }
      }
      if (K.mode == ACM_TOKENS_GAP_SYMBOL) {
        const uint32_t len = (uint32_t)(hi - lo);
        for (uint32_t p = threadIdx.x; p < len; p += blockDim.x) {
          if (!(((S.st[p >> 5] & ~S.ms[p >> 5]) >> (p & 31)) & 1))
            continue;
          const unsigned long long r = rank (p);
          if (r < K.token_capacity) {
            const uint64_t i = lo + p;
            const uint32_t v = K.sb == 1 ? K.text[i] : reinterpret_cast<const unsigned short *> (K.text)[i];
            K.tok_id[r] = K.gap_base + v;
            if (K.tok_start)
              K.tok_start[r] = i + K.pos_base;
            if (K.tok_len)
              K.tok_len[r] = 1;
          }
        }
      } else if (K.mode == ACM_TOKENS_GAP_RUN) {
        /* what ends a run that leaves the tile: the next record, the next text, the end of the buffer */
        uint64_t behind = K.n_symbols;
        if (c1 < n) {
          uint64_t s, e;
          uint32_t len, kw;
          tokens_fact (K, c1, s, e, len, kw);
          behind = s < behind ? s : behind;
        }
        if (K.offsets && k1 <= K.n_texts) {
          const uint64_t o = K.offsets[k1];
          behind = o < behind ? o : behind;
        }
        for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
          uint32_t gap = S.st[w] & ~S.ms[w];
          while (gap) {
            const uint32_t b = (uint32_t)__ffs (gap) - 1;
            gap &= gap - 1;
            const uint32_t p = w * 32 + b;
            uint32_t ww = w, m = (S.cov[w] | S.ts[w]) & (b == 31 ? 0u : ~0u << (b + 1));
            while (!m && ++ww < words)
              m = S.cov[ww] | S.ts[ww];
            const uint64_t run_end = m ? lo + ww * 32 + ((uint32_t)__ffs (m) - 1) : behind;
            const unsigned long long r = rank (p);
            if (r < K.token_capacity) {
              const uint64_t run = run_end - (lo + p);
              K.tok_id[r] = K.gap_base;
              if (K.tok_start)
                K.tok_start[r] = lo + p + K.pos_base;
              if (K.tok_len)
                K.tok_len[r] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)run;
            }
          }
        }
      }
    }
    __syncthreads (); /* (the next tile goes into the same LDS) */
  }
  if (WRITE && K.tok_first) { /* the texts that begin at the end of the buffer: behind every token */
    __shared__ unsigned long long s_tail;
    if (threadIdx.x < WAVE) {
      auto offset = [&] (uint64_t i) { return (uint64_t)K.offsets[i]; };
      const uint64_t kn = K.n_symbols ? tokens_wave_count_le (offset, K.n_texts + 1, K.n_symbols - 1) : 0;
      if (threadIdx.x == 0)
        s_tail = kn;
    }
    __syncthreads ();
    for (uint64_t k = s_tail + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= K.n_texts; k += (uint64_t)gridDim.x * blockDim.x)
      K.tok_first[k] = total;
  }
}
