/* dev_chains.h -- keyword chains with bounded gaps: CHAINS of a record set (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * CHAINS is a function of a record set in canonical order and of offsets[] (no scan kernel touched, no
 * symbol loaded).  The compiled set is an index inverted by keyword: a keyword's postings are the
 * places (chain, level j) it holds in the chains, each with its gaps, the keyword of the level in front
 * and the index of the posting (chain, j - 1) among that keyword's postings.  Every record has one
 * state slot per posting of its keyword, at record index * stride + posting index (stride = the most
 * postings of a keyword, so the room is a function of the arguments alone); a slot holds S + 1 for the
 * greatest start S of an embedding of the chain's terms 0 .. j that ends in this record, 0 for "none",
 * so that the best of a window is a plain maximum.  Tiles of K.tile records (a multiple of 64), blocks
 * stride over the tiles, a wave takes 64 consecutive records at a time.  Behind offsets_check_kernel
 * (dev_batch.h: the batch contract on offsets[] in a launch of its own):
 *   1. chains_level_kernel, once per level j of the set (max_terms launches): the lanes whose keyword
 *      has a posting of level j fill its slot.  Level 0 writes the record's own start.  Level j >= 1:
 *      the window of a record that begins at s is the records that end in [s - 1 - gap_max,
 *      s - 1 - gap_min] (clamped at 0, empty when s <= gap_min); one bisection of the records finds its
 *      first record, and the walk goes forward from there: of every record with the keyword of level
 *      j - 1 the slot the launch before wrote, the maximum kept.
 *      LANE FORM: the lane walks its own window -- windows of up to K.coop records.
 *      WAVE FORM: a lane whose window holds more (the record K.coop places behind the window's first
 *      still ends inside it: one load) waits; the wave then takes these lanes one at a time
 *      (__ballot, the bounds by __shfl), all 64 lanes stride the window with one 16-byte record load
 *      each, and the maximum is reduced across the wave with __shfl_xor.  Every loop around a
 *      cross-lane operation is uniform in the wave.
 *      A record that breaks the contract gets "none" in every slot, so that it takes part in nothing.
 *   2. chains_count_kernel: count[i] = the last-term postings of record i whose slot holds a start
 *      that lies in the text of the record's end (a bisection of offsets[]).  Contract-breaking
 *      records raise the plan's error flag here.
 *   3. a 64-bit exclusive sum (hipCUB) over the capacity + 1 counts: first[].
 *   4. chains_fill_kernel: match j of record i at first[i] + j in posting order, one 16-byte store;
 *      slots at or beyond out_capacity are not written.  One lane writes *d_count.
 *   5. patterns_order_kernel (dev_patterns.h, as it is): the matches of one end come from several
 *      records and chains; every group of equal end_pos is put into (length descending, chain id
 *      ascending).
 * Every slot is written by one lane in each pass; no atomics.  Launch geometry and launch count never
 * depend on what the records hold: capped grids, grid-stride loops.  Bisections and walks are bounded
 * by the record count, so input that is not in canonical order reads nothing out of bounds. */
constexpr uint32_t CHAINS_THREADS = 256;
constexpr uint32_t CHAINS_TILE_DEFAULT = 4096, CHAINS_TILE_MIN = 64, CHAINS_TILE_MAX = 1u << 20; /* records */
constexpr uint32_t CHAINS_COOP_DEFAULT = 64; /* records: one wave-wide load */
constexpr uint32_t CHAINS_LAST = 0x80000000u; /* ChainPost::level: the chain's last term */

/* a place of a keyword in a chain (two 16-byte loads) */
struct ChainPost {
  uint32_t chain, level;      /* level | CHAINS_LAST */
  uint32_t gap_min, gap_max;
  uint32_t prev_kw, prev_idx; /* level >= 1: the keyword of level - 1 and the index of (chain, level - 1) among its postings */
  uint32_t pad[2];
};
static_assert (sizeof (ChainPost) == 32, "two uint4");

struct ChainsK : JoinK {
  /* the compiled set (ACMChains) */
  const uint32_t *post_ptr; /* [n_keywords + 1] the postings of a keyword, by level then chain */
  const ChainPost *post;
  uint32_t n_keywords;
  uint32_t stride;           /* state slots per record: the most postings of a keyword (at least 1) */
  uint32_t level;            /* the level this launch fills */
  uint32_t coop;             /* windows of more records are walked by the wave */
  unsigned long long *state; /* [capacity * stride] S + 1, or 0 */
};

/* the records the passes work on: none after an overflowing scan and under bad offsets */
__device__ __forceinline__ uint64_t
chains_n (const ChainsK &K) {
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  return n_raw > K.capacity || K.ctl->bad ? 0 : n_raw;
}

/* the postings [begin, end) of record r's keyword (none for a keyword the plan got after the set was made); `bad` says whether
 * the record breaks the contract -- it has its postings all the same (join_postings gives it none), and the passes test `bad` */
__device__ __forceinline__ void
chains_postings (const ChainsK &K, const uint4 r, uint32_t &begin, uint32_t &end, bool &bad) {
  begin = end = 0;
  bad = record_breaks_contract (((uint64_t)r.y << 32) | r.x, r.z, K.pos_base, K.n_symbols);
  if (r.w < K.n_keywords) {
    begin = K.post_ptr[r.w];
    end = K.post_ptr[r.w + 1];
  }
}

__device__ __forceinline__ uint64_t
chains_end_of (const ACMRecord *in, uint64_t i) {
  const uint2 p = *reinterpret_cast<const uint2 *> (&in[i]);
  return ((uint64_t)p.y << 32) | p.x;
}

/* the first record of in[0 .. n) that ends at or behind end_pos */
__device__ __forceinline__ uint64_t
chains_first_at (const ACMRecord *in, uint64_t n, uint64_t end_pos) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (chains_end_of (in, mid) < end_pos)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint64_t
chains_shfl64 (uint64_t v, int src) {
  return ((uint64_t)__shfl ((uint32_t)(v >> 32), src, WAVE) << 32) | __shfl ((uint32_t)v, src, WAVE);
}

/* pass 1, once per level */
__global__ __launch_bounds__ (CHAINS_THREADS) void
chains_level_kernel (ChainsK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = chains_n (K);
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) no record here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += CHAINS_THREADS) { /* (uniform in the wave) */
      const uint64_t i = i0 + lane;
      uint4 r = make_uint4 (0, 0, 0, 0);
      uint32_t q = 0, q_end = 0, q0 = 0;
      bool bad = false;
      if (i < n) {
        r = *reinterpret_cast<const uint4 *> (&K.in[i]);
        chains_postings (K, r, q, q_end, bad);
        q0 = q;
      }
      const uint64_t s = (((uint64_t)r.y << 32) | r.x) - K.pos_base + 1 - r.z; /* (used when !bad) */
      for (; __ballot (q < q_end); q++) { /* (uniform in the wave) */
        ChainPost p{};
        bool mine = false;
        if (q < q_end) {
          const uint4 a = reinterpret_cast<const uint4 *> (&K.post[q])[0];
          p.chain = a.x;
          p.level = a.y;
          p.gap_min = a.z;
          p.gap_max = a.w;
          mine = (p.level & ~CHAINS_LAST) == K.level;
        }
        unsigned long long best = 0;
        bool wide = false;
        uint64_t w = 0, hi = 0; /* the window: its first record, the last end (a position) inside it */
        if (mine && !bad && K.level == 0)
          best = s + 1;
        else if (mine && !bad && s > p.gap_min) {
          const uint2 b = reinterpret_cast<const uint2 *> (&K.post[q])[2];
          p.prev_kw = b.x;
          p.prev_idx = b.y;
          hi = K.pos_base + s - 1 - p.gap_min;
          w = chains_first_at (K.in, n, K.pos_base + (s - 1 >= p.gap_max ? s - 1 - p.gap_max : 0));
          wide = w < n && n - w > K.coop && chains_end_of (K.in, w + K.coop) <= hi; /* more than K.coop records inside */
          if (!wide)
            for (; w < n; w++) {
              const uint4 o = *reinterpret_cast<const uint4 *> (&K.in[w]);
              if ((((uint64_t)o.y << 32) | o.x) > hi)
                break;
              if (o.w == p.prev_kw) {
                const unsigned long long v = K.state[w * K.stride + p.prev_idx];
                best = v > best ? v : best;
              }
            }
        }
        for (uint64_t todo = __ballot (wide); todo; todo &= todo - 1) { /* (uniform in the wave) */
          const int src = __ffsll ((unsigned long long)todo) - 1;
          const uint64_t w_src = chains_shfl64 (w, src), hi_src = chains_shfl64 (hi, src);
          const uint32_t kw_src = __shfl (p.prev_kw, src, WAVE), idx_src = __shfl (p.prev_idx, src, WAVE);
          unsigned long long top = 0;
          for (uint64_t at = w_src;; at += WAVE) { /* (uniform in the wave: at < n at its first round) */
            const uint64_t x = at + lane;
            bool inside = x < n;
            if (inside) {
              const uint4 o = *reinterpret_cast<const uint4 *> (&K.in[x]);
              inside = (((uint64_t)o.y << 32) | o.x) <= hi_src;
              if (inside && o.w == kw_src) {
                const unsigned long long v = K.state[x * K.stride + idx_src];
                top = v > top ? v : top;
              }
            }
            if (__ballot (inside) != ~0ull) /* the window ends in this round */
              break;
          }
          for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned long long other = chains_shfl64 (top, (int)lane ^ d);
            top = other > top ? other : top;
          }
          if ((int)lane == src)
            best = top;
        }
        if (mine)
          K.state[i * K.stride + (q - q0)] = best;
      }
    }
  }
}

/* the chain match that posting p (a last term) of a record that ends at buffer index e gives from its slot value v: whether there
 * is one, and its first symbol S */
__device__ __forceinline__ bool
chains_match (const ChainsK &K, uint64_t e, unsigned long long v, uint64_t &S) {
  if (v == 0 || v - 1 > e)
    return false;
  S = v - 1;
  if (K.offsets) { /* (uniform; checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols, and there are texts) */
    const uint64_t t = batch_text_of (K.offsets, 0, K.n_texts - 1, S);
    if (e >= K.offsets[t + 1]) /* the match would span a cut */
      return false;
  }
  return true;
}

/* pass 2 */
__global__ __launch_bounds__ (CHAINS_THREADS) void
chains_count_kernel (ChainsK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = chains_n (K);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    K.ctl->n = n;
    K.count[K.capacity] = 0; /* (the prefix sum reads capacity + 1 entries) */
  }
  bool any_bad = false;
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += CHAINS_THREADS) {
      const uint64_t i = i0 + lane;
      uint32_t found = 0;
      if (i < n) {
        const uint4 r = *reinterpret_cast<const uint4 *> (&K.in[i]);
        uint32_t q = 0, q_end = 0;
        bool bad = false;
        chains_postings (K, r, q, q_end, bad);
        any_bad = any_bad || bad;
        const uint64_t e = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
        for (uint32_t q0 = q; !bad && q < q_end; q++)
          if (K.post[q].level & CHAINS_LAST) {
            uint64_t S;
            found += chains_match (K, e, K.state[i * K.stride + (q - q0)], S);
          }
      }
      if (i < end)
        K.count[i] = found;
    }
  }
  if (any_bad && K.error)
    *K.error = 1;
}

/* pass 3 */
__global__ __launch_bounds__ (CHAINS_THREADS) void
chains_fill_kernel (ChainsK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = K.ctl->n;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_count = K.first[K.capacity];
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) no record here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += CHAINS_THREADS) {
      const uint64_t i = i0 + lane;
      if (i >= n)
        continue;
      unsigned long long at = K.first[i];
      const unsigned long long at_end = K.first[i + 1];
      if (at == at_end)
        continue;
      const uint4 r = *reinterpret_cast<const uint4 *> (&K.in[i]);
      uint32_t q = 0, q_end = 0;
      bool bad = false;
      chains_postings (K, r, q, q_end, bad);
      const uint64_t e = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
      for (uint32_t q0 = q; q < q_end && at < at_end; q++) { /* (at < at_end always: pass 2 counted the same matches) */
        const ChainPost &p = K.post[q];
        if (!(p.level & CHAINS_LAST))
          continue;
        uint64_t S;
        if (!chains_match (K, e, K.state[i * K.stride + (q - q0)], S))
          continue;
        if (at < K.out_capacity)
          *reinterpret_cast<uint4 *> (&K.out[at]) = make_uint4 (r.x, r.y, (uint32_t)(e + 1 - S), p.chain);
        at++;
      }
    }
  }
}
