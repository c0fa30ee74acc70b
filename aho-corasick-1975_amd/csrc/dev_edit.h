/* dev_edit.h -- keywords within edit distance k: EDIT of a record set (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The compiled set, the kernel arguments (ApproxK), the check of offsets[], the prefix sum and the order passes
 * are dev_approx.h's; the group routine is new.  A seed -- record end q of term j (offset o, length l) of target
 * w, r = L - o - l symbols of the target behind the piece -- no longer fixes one start: it fixes the ends
 * e0 = q + max (0, r - k) .. e1 = min (q + r + k, hi - 1) and a band of start diagonals.  One GROUP of G
 * consecutive lanes takes one input record, G = 16, 32 or 64 for a set's max_k <= 3, 7 or 15 (the band is at most
 * 4 k + 1 = 13, 29 or 61 diagonals wide); tiles of K.tile records, blocks stride over the tiles.  Per posting:
 *   1. the cheap tests, the same in all lanes of the group: the term's length is the record's, the text [lo, hi)
 *      of q by a bisection of offsets[], the piece begins at or behind lo, e0 <= e1.
 *   2. the banded dynamic programme.  Cell (i, c): i symbols of the target matched, the text consumed up to c;
 *      lane d holds the diagonal c - i = B + d, B = e0 + 1 - L - k.  A cell is cost << 6 | (63 - d0), d0 the
 *      lane whose row-0 cell its path began in, so one unsigned minimum takes the least cost and then the
 *      largest start.  Cells above k, left of lo, right of e1 + 1 and outside the band are EDIT_INF.  The cells
 *      are computed as an ANTI-DIAGONAL WAVEFRONT: at step T lane d computes its row i = (T - d) / 2 when T - d
 *      is even, from its own last value (the diagonal neighbour, two steps old) and the last values of lanes
 *      d + 1 (above) and d - 1 (left), both one step old -- two independent cross-lane reads per step and no
 *      scan, 2 L + band steps (DESIGN.md 4.24 has the reasoning against the row-by-row prefix minimum).  The
 *      text and spelling symbols of a lane's next row are loaded when it finishes a row, two steps ahead of
 *      their use: naturally aligned loads of one symbol, consecutive lanes on consecutive text symbols.
 *      Ukkonen's cut-off: the group stops once no lane that still has a row to compute, or that finished in
 *      this very step (its value is the left neighbour of the next lane's last row), is within the budget.
 *      The step loop is wave-uniform (it runs to the longest of the wave's groups, finished groups predicated
 *      off), so every shuffle and ballot is executed by all 64 lanes.  Behind row L lane d holds
 *      (D_w (e), s*_w (e)) of e = e0 - k + d, for every e in [e0, e1] whose D is within the budget.
 *   3. ownership: (w, e) is emitted by the least (term index, record end) among the seeds that satisfy the seed
 *      condition for e.  The group tests, per end it found, every term j' < j with every e - q' in
 *      [max (0, r' - k), r' + k], and its own term with q' < q: at most (k + 1)(2 k + 1) independent lookups
 *      (records_have of dev_patterns.h), dealt to the group's lanes and combined with a ballot.  It depends on
 *      the input alone, so each (w, e) comes out once and the count is exact without a list of candidates.  It
 *      stands behind the dynamic programme, since few candidates get that far.
 * edit_count_kernel, the 64-bit exclusive sum, edit_fill_kernel (the groups with a nonzero count verify again;
 * lane 0 of the group stores match m of record i at first[i] + m, in ascending e) and dev_approx.h's order
 * passes follow; K.longest is the longest L plus max_k there, since a match may be longer than its target.
 * Every slot is written by one lane in each pass; no atomics.  Launch geometry never depends on what the
 * records hold: capped grids, blocks striding over tiles. */
constexpr uint32_t EDIT_THREADS = 256, EDIT_MAX_K = 15;
constexpr uint32_t EDIT_TILE_DEFAULT = 64, EDIT_TILE_MIN = 64, EDIT_TILE_MAX = 1u << 20; /* records */
constexpr uint32_t EDIT_INF = 0x0FFFFFFFu; /* (+ 64 does not wrap; above every cell within a budget of 15) */

/* What a wave does with its 64 / G records: every group walks the postings [q, q_end) of its record r (none:
 * q == q_end) and returns the number of matches it owns; with FILL it stores them from slot `at` on.  All 64
 * lanes call this together; q, q_end, r and `at` are the same in the G lanes of a group. */
template <typename T, uint32_t G, bool FILL>
__device__ __forceinline__ uint32_t
edit_group (const ApproxK &K, uint64_t n, const uint4 r, uint32_t q, uint32_t q_end, unsigned long long at) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), sub = lane & (G - 1), shift = lane & ~(G - 1);
  const uint64_t group_bits = G == WAVE ? ~0ull : (1ull << (G & 63)) - 1;
  const T *__restrict__ text = static_cast<const T *> (K.text);
  const uint64_t eq = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
  uint32_t found = 0;
  while (__ballot (q < q_end)) { /* (uniform in the wave) */
    /* 1. */
    bool cand = false;
    uint32_t L = 0, k = 0, w = 0, j = 0, first_term = 0, nd = 0, span = 0; /* nd: diagonals of the band; span = e1 - e0 */
    uint64_t e0 = 0, t_lo = 0;
    int64_t c0 = 0, c_lo = 0, c_hi = -1; /* c0: this lane's column in row 0; cells exist for columns [c_lo, c_hi] */
    const T *__restrict__ spell = nullptr;
    if (q < q_end) {
      const uint4 p = K.post[q++];
      if (r.z == p.w) { /* the piece's length */
        const uint4 tg = K.target[p.x];
        uint64_t t_hi = K.n_symbols;
        if (K.offsets) { /* (uniform; checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols, and there are texts) */
          const uint64_t t = batch_text_of (K.offsets, 0, K.n_texts - 1, eq);
          t_lo = K.offsets[t];
          t_hi = K.offsets[t + 1];
        }
        const uint32_t behind = tg.x - p.z - p.w;
        if (eq + 1 >= t_lo + p.w && eq < t_hi) { /* the piece lies inside the text of its end (else: a record that spans a cut) */
          const uint64_t e1 = eq + behind + tg.y < t_hi - 1 ? eq + behind + tg.y : t_hi - 1;
          e0 = eq + (behind > tg.y ? behind - tg.y : 0);
          if (e0 <= e1) {
            cand = true;
            w = p.x;
            j = p.y;
            L = tg.x;
            k = tg.y;
            first_term = tg.z;
            span = (uint32_t)(e1 - e0);
            nd = span + 2 * k + 1;
            c0 = (int64_t)e0 + 1 - (int64_t)L - (int64_t)k + sub;
            c_lo = (int64_t)t_lo;
            c_hi = (int64_t)e1 + 1;
            spell = static_cast<const T *> (K.spell) + K.spell_off[w];
          }
        }
      }
    }
    /* 2. row 0, and the symbols of row 1 */
    const bool banded = cand && sub < nd;
    uint32_t cur = banded && c0 >= c_lo && c0 <= c_hi ? 63 - sub : EDIT_INF;
    const uint64_t steps = cand ? 2 * (uint64_t)L + nd - 1 : 0;
    uint64_t i = 1, next_step = (uint64_t)sub + 2; /* the row this lane computes next, and the step it does so in */
    T ts = 0, ps = 0;
    if (banded && c0 >= c_lo && c0 < c_hi) {
      ts = text[c0];
      ps = spell[0];
    }
    bool live = cand;
    for (uint64_t step = 1;; step++) { /* (uniform in the wave: to the longest of its groups) */
      const bool on = live && step <= steps;
      if (!__ballot (on))
        break;
      uint32_t up = __shfl_down (cur, 1, G), left = __shfl_up (cur, 1, G);
      if (sub == G - 1)
        up = EDIT_INF;
      if (sub == 0)
        left = EDIT_INF;
      if (on && banded && step == next_step && i <= L) {
        const int64_t c = c0 + (int64_t)i;
        uint32_t v = EDIT_INF;
        if (c >= c_lo && c <= c_hi) {
          const uint32_t side = (up < left ? up : left) + 64, diag = cur + (ts != ps ? 64 : 0);
          v = diag < side ? diag : side;
          if ((v >> 6) > k)
            v = EDIT_INF;
        }
        cur = v;
        if (i < L && c >= c_lo && c < c_hi) { /* row i + 1 compares text[c] with spell[i] */
          ts = text[c];
          ps = spell[i];
        }
        i++;
        next_step += 2;
      }
      const bool within = banded && cur != EDIT_INF && 2 * (uint64_t)L + sub >= step; /* (a finished lane counts in its last step only) */
      live = on && ((__ballot (within) >> shift) & group_bits) != 0;
    }
    /* 3. the ends found, in ascending e */
    uint64_t todo = (__ballot (banded && sub >= k && sub <= k + span && cur != EDIT_INF) >> shift) & group_bits;
    while (__ballot (todo != 0)) { /* (uniform in the wave) */
      const bool has = todo != 0;
      const uint32_t d = has ? (uint32_t)__ffsll ((unsigned long long)todo) - 1 : 0;
      todo &= todo - 1;
      const uint64_t e = e0 + d - k;
      bool lower = false;
      if (has) {
        const uint32_t per = 2 * k + 1, lookups = (j + 1) * per;
        for (uint32_t x = sub; x < lookups && !lower; x += G) {
          const uint32_t jj = x / per;
          const ApproxTerm o = K.terms[first_term + jj];
          const int64_t back = (int64_t)(L - o.offset - o.length) - (int64_t)k + (int64_t)(x % per); /* e - q' */
          if (back < 0 || (uint64_t)back > e)
            continue;
          const uint64_t qq = e - (uint64_t)back;
          if (qq + 1 < t_lo + o.length || (jj == j && qq >= eq)) /* the piece begins in front of lo; of the own term only q' < q */
            continue;
          lower = records_have (K.in, n, K.pos_base + qq, o.length, o.keyword_id);
        }
      }
      const bool owned = has && ((__ballot (lower) >> shift) & group_bits) == 0;
      const uint32_t cell = __shfl (cur, d, G);
      if (owned) {
        if (FILL) {
          if (sub == 0 && at < K.out_capacity) {
            const uint64_t end_pos = K.pos_base + e;
            *reinterpret_cast<uint4 *> (&K.fill[at]) = make_uint4 ((uint32_t)end_pos, (uint32_t)(end_pos >> 32), L + d - (63 - (cell & 63)), w);
            K.fill_dist[at] = cell >> 6;
          }
          at++;
        }
        found++;
      }
    }
  }
  return found;
}

/* pass 1 */
template <typename T, uint32_t G>
__global__ __launch_bounds__ (EDIT_THREADS) void
edit_count_kernel (ApproxK K) {
  constexpr uint32_t PER_WAVE = WAVE / G, PER_BLOCK = EDIT_THREADS / G;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, group = lane / G;
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  const uint64_t n = n_raw > K.capacity || K.ctl->bad ? 0 : n_raw; /* an overflowing scan left nothing to verify */
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    K.ctl->n = n;
    K.count[K.capacity] = 0; /* (the prefix sum reads capacity + 1 entries) */
  }
  bool bad = false;
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * PER_WAVE; i0 < end; i0 += PER_BLOCK) { /* (uniform in the wave) */
      const uint64_t i = i0 + group;
      uint4 r = make_uint4 (0, 0, 0, 0);
      uint32_t q = 0, q_end = 0;
      if (i < n) {
        r = *reinterpret_cast<const uint4 *> (&K.in[i]);
        join_postings (K, K.post_ptr, K.n_keywords, r, q, q_end, bad);
      }
      const uint32_t found = edit_group<T, G, false> (K, n, r, q, q_end, 0);
      if (i < end && (lane & (G - 1)) == 0)
        K.count[i] = found;
    }
  }
  if (bad && K.error)
    *K.error = 1;
}

/* pass 2 */
template <typename T, uint32_t G>
__global__ __launch_bounds__ (EDIT_THREADS) void
edit_fill_kernel (ApproxK K) {
  constexpr uint32_t PER_WAVE = WAVE / G, PER_BLOCK = EDIT_THREADS / G;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, group = lane / G;
  const uint64_t n = K.ctl->n;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_count = K.first[K.capacity];
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) no record here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * PER_WAVE; i0 < end; i0 += PER_BLOCK) {
      const uint64_t i = i0 + group;
      uint4 r = make_uint4 (0, 0, 0, 0);
      uint32_t q = 0, q_end = 0;
      unsigned long long at = 0;
      if (i < n) {
        at = K.first[i];
        if (at != K.first[i + 1]) { /* (else: pass 1 found no match here) */
          bool bad = false;
          r = *reinterpret_cast<const uint4 *> (&K.in[i]);
          join_postings (K, K.post_ptr, K.n_keywords, r, q, q_end, bad);
        }
      }
      (void)edit_group<T, G, true> (K, n, r, q, q_end, at);
    }
  }
}
