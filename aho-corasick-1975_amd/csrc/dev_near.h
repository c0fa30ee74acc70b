/* dev_near.h -- unordered keyword proximity: NEAR of a record set (include/acm_near.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * NEAR is a function of a record set in canonical order and of offsets[] (no scan kernel touched, no
 * symbol loaded).  The compiled set is an index inverted by keyword: a keyword's postings are the
 * places (group, term index j) it holds in the groups, each with the group's width, need and number of
 * terms m, sorted by group.  Every record has one slot per posting of its keyword, at record index *
 * stride + posting index (stride = the most postings of a keyword, so the room is a function of the
 * arguments alone); a slot holds S* + 1 of (group, the record's end), or 0.  Tiles of K.tile records (a
 * multiple of 64), blocks stride over the tiles, a wave takes 64 consecutive records at a time.  Behind
 * offsets_check_kernel (dev_batch.h: the batch contract on offsets[] in a launch of its own):
 *   1. near_walk_kernel, ONE launch.  The HEAD of (g, e) is the first record in canonical order that
 *      ends at e, keeps the contract and has a keyword of g; only its lane computes S*, the slots of
 *      the other records of g at e are 0, so there is one output per (g, e) without a pass that
 *      removes doubles.  Records of equal end are adjacent: the head test is a look backwards over
 *      them, one bisection of a keyword's few postings per record ("which term of g, if any").
 *      The head finds the last record that ends at e and the begin of e's text once (one bisection of
 *      offsets[]), then walks the records BACKWARDS from there and keeps, per term u of g, the
 *      distance e + 1 - s of the greatest start s seen (0: none) and a mask of the terms that end at
 *      e (the anchors).  A start in front of lo = max (text begin, e + 1 - width) is dropped at once:
 *      a cover with it would begin in front of lo, which none may.  Hence a distance is at most
 *      width <= 2^20, and e + 1 - width is never formed.  Records of one keyword have one length, so
 *      a term's best start at an end where it anchors IS its anchor's start, and the closed form of
 *      the header reads one column: S* = the greatest over the anchors a of min (best_a, the (need -
 *      1)-th greatest best_u, u != a), recomputed when a best_u or the mask changes.
 *      THE EXIT.  The walk stops at the first record whose end lies in front of lo (ends descend:
 *      every record further back ends, and so begins, in front of lo too) or at or in front of the
 *      current S*.  For the second: every record further back begins at or in front of that end,
 *      hence at or in front of S*.  Let a best_u rise to v <= S*.  For an anchor a the (need - 1)-th
 *      greatest of the others either stays or becomes a value <= v, and so every S_a either stays or
 *      becomes a value <= max (old S_a, v) <= S*; the anchor that gave S* keeps its S_a, because the
 *      need - 1 values that stood at or above S* still do.  A new anchor cannot appear (anchors end
 *      at e > S* - 1).  So S* is final.  In a dense record set the walk is as long as the answer's
 *      span, not as the width window; a forward walk of the whole window would be quadratic there.
 *      LANE FORM: the head walks up to K.coop records itself.
 *      WAVE FORM: a head whose walk is still running then waits; the wave takes these lanes one at a
 *      time (__ballot, the bounds by __shfl), 64 lanes load the next 64 records per round, the
 *      per-term minima of the round are reduced across the wave with __shfl_xor into the owner's
 *      column, and the owner applies the exit test once per round.  Walking further than the exit
 *      never changes S* (the argument above), so both forms give the same output.  Every loop around
 *      a cross-lane operation is uniform in the wave.
 *      The per-term state is best[16][NEAR_THREADS] in LDS (16 KiB for the block of 256), term-major,
 *      so that the 64 lanes of a wave touch 64 consecutive words and nothing is indexed dynamically
 *      in registers (which would go to scratch memory); a lane only ever touches its own column, so
 *      no barrier is needed.
 *      A record that breaks the contract gets 0 in every slot, is no head, anchors nothing and counts
 *      for no term.
 *   2. near_count_kernel: count[i] = the slots of record i that hold a window.  Contract-breaking
 *      records raise the plan's error flag here.
 *   3. a 64-bit exclusive sum (hipCUB) over the capacity + 1 counts: first[].
 *   4. near_fill_kernel: match j of record i at first[i] + j in posting (that is group) order, one
 *      16-byte store; slots at or beyond out_capacity are not written.  One lane writes *d_count.
 *   5. patterns_order_kernel (dev_patterns.h, as it is): the matches of one end come from several
 *      heads; every group of equal end_pos is put into (length descending, group id ascending).
 * Every slot is written by one lane in each pass; no atomics.  Launch geometry and launch count never
 * depend on what the records hold: capped grids, grid-stride loops.  Bisections and walks are bounded
 * by the record count, so input that is not in canonical order reads nothing out of bounds.
 * NEAR_COOP_DEFAULT is CHAINS' value.  NEAR_TILE_DEFAULT is not: a walk is a chain of dependent loads, so the
 * pass lives on waves in flight, and CHAINS' tile of 4,096 records leaves 555,000 records to 136 blocks.  One
 * wave-round per wave and block (256 records) measured 3 to 6 times faster than 4,096 at every width and
 * threshold, 64 and 1,024 lie between (tools/exp_near.py, profiles/near.json). */
constexpr uint32_t NEAR_THREADS = 256;
constexpr uint32_t NEAR_TILE_DEFAULT = 256, NEAR_TILE_MIN = 64, NEAR_TILE_MAX = 1u << 20; /* records */
constexpr uint32_t NEAR_COOP_DEFAULT = 64; /* records: one wave-wide load */
constexpr uint32_t NEAR_TERMS = 16;        /* ACM_NEAR_TERMS_MAX */

/* a place of a keyword in a group (one 16-byte load) */
struct NearPost {
  uint32_t group, width;
  uint32_t shape; /* term index j | m << 8 | need << 16 (need: 1 .. m) */
  uint32_t pad;
};
static_assert (sizeof (NearPost) == 16, "one uint4");

struct NearK : JoinK {
  /* the compiled set (ACMNear) */
  const uint32_t *post_ptr; /* [n_keywords + 1] the postings of a keyword, by group */
  const NearPost *post;
  uint32_t n_keywords;
  uint32_t stride;           /* slots per record: the most postings of a keyword (at least 1) */
  uint32_t coop;             /* walks of more records are finished by the wave */
  unsigned long long *state; /* [capacity * stride] S* + 1, or 0 */
};

/* the records the passes work on: none after an overflowing scan and under bad offsets */
__device__ __forceinline__ uint64_t
near_n (const NearK &K) {
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  return n_raw > K.capacity || K.ctl->bad ? 0 : n_raw;
}

__device__ __forceinline__ bool
near_bad (const NearK &K, const uint4 r) {
  return record_breaks_contract (((uint64_t)r.y << 32) | r.x, r.z, K.pos_base, K.n_symbols);
}

/* the postings [begin, end) of a keyword (none for one the plan got after the set was made) */
__device__ __forceinline__ void
near_postings (const NearK &K, uint32_t keyword, uint32_t &begin, uint32_t &end) {
  begin = end = 0;
  if (keyword < K.n_keywords) {
    begin = K.post_ptr[keyword];
    end = K.post_ptr[keyword + 1];
  }
}

/* which term of `group` the keyword is: its index, or -1 (a bisection of the keyword's postings, which are sorted by group) */
__device__ __forceinline__ int
near_term_of (const NearK &K, uint32_t keyword, uint32_t group) {
  uint32_t lo, hi;
  near_postings (K, keyword, lo, hi);
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const uint2 p = *reinterpret_cast<const uint2 *> (&K.post[mid]);
    if (p.x == group)
      return (int)(K.post[mid].shape & 0xFF);
    if (p.x < group)
      lo = mid + 1;
    else
      hi = mid;
  }
  return -1;
}

/* the term and the distance e + 1 - s that record o gives the walk of (group, an end at position E), gap = E - o's end being below
 * the walk's limit: -1 for a record that breaks the contract, has no keyword of the group or begins more than dmax - 1 in front of E */
__device__ __forceinline__ int
near_take (const NearK &K, const uint4 o, uint64_t gap, uint32_t group, uint32_t dmax, uint32_t &d) {
  if (near_bad (K, o))
    return -1;
  const uint64_t far = gap + o.z; /* (gap < 2^20 and a 32-bit length: no wrap) */
  if (far > dmax)
    return -1;
  d = (uint32_t)far;
  return near_term_of (K, o.w, group);
}

/* The closed form over one column of the LDS state (col[u * NEAR_THREADS] = term u's least distance, 0: none): the least
 * over the anchors a of max (col[a], the (need - 1)-th least of the others); 0: no cover. */
__device__ __forceinline__ uint32_t
near_window (const uint32_t *col, uint32_t m, uint32_t need, uint32_t anchors) {
  uint32_t D = 0;
  for (uint32_t rest = anchors; rest; rest &= rest - 1) {
    const uint32_t a = (uint32_t)__ffs ((int)rest) - 1;
    uint32_t Da = col[a * NEAR_THREADS];
    if (need > 1) {
      uint32_t kth = 0; /* the one with need - 2 of the others in front of it */
      for (uint32_t u = 0; u < m && !kth; u++) {
        const uint32_t du = col[u * NEAR_THREADS];
        if (u == a || !du)
          continue;
        uint32_t before = 0;
        for (uint32_t v = 0; v < m; v++) {
          const uint32_t dv = col[v * NEAR_THREADS];
          before += v != a && v != u && dv && (dv < du || (dv == du && v < u));
        }
        if (before == need - 2)
          kth = du;
      }
      if (!kth)
        continue;
      Da = kth > Da ? kth : Da;
    }
    D = D == 0 || Da < D ? Da : D;
  }
  return D;
}

/* pass 1 */
__global__ __launch_bounds__ (NEAR_THREADS) void
near_walk_kernel (NearK K) {
  __shared__ uint32_t best[NEAR_TERMS][NEAR_THREADS];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  uint32_t *col = &best[0][threadIdx.x];
  const uint64_t n = near_n (K);
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) no record here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += NEAR_THREADS) { /* (uniform in the wave) */
      const uint64_t i = i0 + lane;
      uint4 r = make_uint4 (0, 0, 0, 0);
      uint32_t q = 0, q_end = 0, q0 = 0;
      bool bad = true;
      if (i < n) {
        r = *reinterpret_cast<const uint4 *> (&K.in[i]);
        near_postings (K, r.w, q, q_end);
        q0 = q;
        bad = near_bad (K, r);
      }
      const uint64_t E = ((uint64_t)r.y << 32) | r.x; /* the record's end, a position */
      /* once per record with a posting: the run [eq_lo, hi] of records that end at E, and how far a window may reach back
       * inside E's text */
      uint64_t eq_lo = i, hi = i, reach = 0;
      if (!bad && q < q_end) {
        while (eq_lo > 0 && chains_end_of (K.in, eq_lo - 1) == E)
          eq_lo--;
        while (hi + 1 < n && chains_end_of (K.in, hi + 1) == E)
          hi++;
        const uint64_t e = E - K.pos_base;
        /* (checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols, and there are texts) */
        reach = e + 1 - (K.offsets ? K.offsets[batch_text_of (K.offsets, 0, K.n_texts - 1, e)] : 0);
      }
      for (; __ballot (q < q_end); q++) { /* (uniform in the wave) */
        uint32_t group = 0, m = 0, need = 0, dmax = 0, anchors = 0, D = 0, lim = 0;
        bool mine = q < q_end, head = false, wide = false;
        uint64_t w = hi;
        if (mine && !bad) {
          const uint4 p = *reinterpret_cast<const uint4 *> (&K.post[q]);
          group = p.x;
          m = (p.z >> 8) & 0xFF;
          need = p.z >> 16;
          dmax = reach < p.y ? (uint32_t)reach : p.y;
          head = true;
          for (uint64_t k = eq_lo; k < i && head; k++) {
            const uint4 o = *reinterpret_cast<const uint4 *> (&K.in[k]);
            head = near_bad (K, o) || near_term_of (K, o.w, group) < 0;
          }
        }
        if (head) {
          for (uint32_t u = 0; u < m; u++)
            col[u * NEAR_THREADS] = 0;
          lim = dmax;
          for (uint64_t steps = 0;; steps++) {
            if (steps >= K.coop) {
              wide = true;
              break;
            }
            const uint4 o = *reinterpret_cast<const uint4 *> (&K.in[w]);
            const uint64_t gap = E - (((uint64_t)o.y << 32) | o.x);
            if (gap >= lim) /* the exit (an end behind E, in input out of order, wraps and leaves too) */
              break;
            uint32_t d = 0;
            const int j = near_take (K, o, gap, group, dmax, d);
            if (j >= 0) {
              const uint32_t cur = col[j * NEAR_THREADS], bit = gap == 0 ? 1u << j : 0;
              if (cur == 0 || d < cur || (bit & ~anchors)) {
                if (cur == 0 || d < cur)
                  col[j * NEAR_THREADS] = d;
                anchors |= bit;
                D = near_window (col, m, need, anchors);
                lim = D ? D - 1 : dmax;
              }
            }
            if (w == 0)
              break;
            w--;
          }
        }
        for (uint64_t todo = __ballot (wide); todo; todo &= todo - 1) { /* (uniform in the wave) */
          const int src = __ffsll ((unsigned long long)todo) - 1;
          const uint64_t E_src = chains_shfl64 (E, src);
          const uint32_t group_src = __shfl (group, src, WAVE), dmax_src = __shfl (dmax, src, WAVE), m_src = __shfl (m, src, WAVE);
          uint64_t w_src = chains_shfl64 (w, src);
          for (bool done = false; !done;) { /* (uniform in the wave) */
            const uint32_t lim_src = __shfl (lim, src, WAVE);
            bool inside = lane <= w_src;
            int j = -1;
            uint32_t d = 0;
            bool at_end = false;
            if (inside) {
              const uint4 o = *reinterpret_cast<const uint4 *> (&K.in[w_src - lane]);
              const uint64_t gap = E_src - (((uint64_t)o.y << 32) | o.x);
              inside = gap < lim_src;
              if (inside) {
                j = near_take (K, o, gap, group_src, dmax_src, d);
                at_end = gap == 0;
              }
            }
            bool changed = false;
            for (uint32_t u = 0; u < m_src; u++) { /* (uniform in the wave) */
              uint32_t least = j == (int)u ? d : ~0u;
              for (int x = 1; x < WAVE; x <<= 1) {
                const uint32_t other = __shfl (least, (int)lane ^ x, WAVE);
                least = other < least ? other : least;
              }
              const bool anchored = __ballot (j == (int)u && at_end) != 0;
              if ((int)lane == src) {
                const uint32_t cur = col[u * NEAR_THREADS], bit = anchored ? 1u << u : 0;
                if (least != ~0u && (cur == 0 || least < cur)) {
                  col[u * NEAR_THREADS] = least;
                  changed = true;
                }
                changed = changed || (bit & ~anchors);
                anchors |= bit;
              }
            }
            if ((int)lane == src && changed) {
              D = near_window (col, m, need, anchors);
              lim = D ? D - 1 : dmax;
            }
            /* the walk ends in the round that met a record outside the limit or the first record */
            done = __ballot (inside) != ~0ull || w_src < WAVE;
            w_src -= done ? 0 : WAVE;
          }
        }
        if (mine) /* (D <= dmax <= e + 1: the window begins inside the buffer and inside e's text) */
          K.state[i * K.stride + (q - q0)] = head && D ? E - K.pos_base + 1 - D + 1 : 0;
      }
    }
  }
}

/* pass 2 */
__global__ __launch_bounds__ (NEAR_THREADS) void
near_count_kernel (NearK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = near_n (K);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    K.ctl->n = n;
    K.count[K.capacity] = 0; /* (the prefix sum reads capacity + 1 entries) */
  }
  bool any_bad = false;
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += NEAR_THREADS) {
      const uint64_t i = i0 + lane;
      uint32_t found = 0;
      if (i < n) {
        const uint4 r = *reinterpret_cast<const uint4 *> (&K.in[i]);
        uint32_t q = 0, q_end = 0;
        near_postings (K, r.w, q, q_end);
        const bool bad = near_bad (K, r);
        any_bad = any_bad || bad;
        for (uint32_t q0 = q; !bad && q < q_end; q++)
          found += K.state[i * K.stride + (q - q0)] != 0;
      }
      if (i < end)
        K.count[i] = found;
    }
  }
  if (any_bad && K.error)
    *K.error = 1;
}

/* pass 3 */
__global__ __launch_bounds__ (NEAR_THREADS) void
near_fill_kernel (NearK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = K.ctl->n;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_count = K.first[K.capacity];
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) no record here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += NEAR_THREADS) {
      const uint64_t i = i0 + lane;
      if (i >= n)
        continue;
      unsigned long long at = K.first[i];
      const unsigned long long at_end = K.first[i + 1];
      if (at == at_end)
        continue;
      const uint4 r = *reinterpret_cast<const uint4 *> (&K.in[i]);
      uint32_t q = 0, q_end = 0;
      near_postings (K, r.w, q, q_end);
      const uint64_t e = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
      for (uint32_t q0 = q; q < q_end && at < at_end; q++) { /* (at < at_end always: pass 2 counted the same slots) */
        const unsigned long long v = K.state[i * K.stride + (q - q0)];
        if (v == 0)
          continue;
        if (at < K.out_capacity)
          *reinterpret_cast<uint4 *> (&K.out[at]) = make_uint4 (r.x, r.y, (uint32_t)(e + 1 - (v - 1)), K.post[q].group);
        at++;
      }
    }
  }
}
