/* dev_segment.h -- the minimum-cost tiling: SEGMENT of a record set (include/acm_segment.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * SEGMENT is a function of the RECORDS alone, as SELECT is: it runs behind the ordered scan of any
 * plan kind and touches no scan kernel.  The rule is a shortest path over the positions and
 * sequential by its wording, but it decomposes at CUTS: a cut is a position no record spans.  Across
 * a cut best[] is additive -- every path goes through the cut --, so the comparisons of step 2 and
 * the equality tests of step 3 on one side of it do not change when best[] of the other side is
 * shifted by a constant: every maximal GROUP of records chained by shared symbols is a problem of its
 * own, with best = 0 at the cut in front of it.  The records stay in canonical order (no order
 * pass, so no host round trip for any record set); with i, j indices in that order:
 *   a. select_key_kernel and select_drop_kernel (dev_select.h, SELECT's own validation: the records
 *      become (start, length, keyword_id) in scratch, those that break the contract go out), then
 *      segment_check_kernel: a keyword_id >= n_keywords or a cost of 2^24 or more stops the call
 *      (SegmentCtl::fatal) before any cost is read through a keyword_id and before any sum is made.
 *   b. groups.  Record i begins a group iff the minimum start over i and all later records exceeds
 *      the end of record i - 1 (ends ascend, so that is the largest end in front).  dev_context.h's
 *      MERGE test and its shape: segment_min_kernel (the tiles' minima), segment_carry_kernel (one
 *      block: suffix minima over the tiles), segment_flag_kernel (the suffix minimum inside a tile,
 *      backwards, carried in; mark[i] bit 0 and the tile's count), the exclusive sum over the tiles,
 *      segment_place_kernel<false> (group_first[]: select_cand_kernel's COUNT / sum / WRITE).
 *   c. segment_link_kernel, fully parallel: prev (i) = the last record j with end_j < start_i (it is
 *      the last of its end class), by a gallop backwards from i and a bisection over the ascending
 *      ends.  A prev in front of the group counts as none.
 *   d. the forward recurrence per group, base = the cut in front of it:
 *        W_i = (prev: V[prev] + gap * (start_i - end_prev - 1), none: gap * (start_i - base)) + cost_i
 *        V_i = min (V_{i-1} + gap * (end_i - end_{i-1}), W_i)            (64-bit)
 *      so V of the last record of an end class is best[end + 1].  Every record notes which record
 *      of its class so far attains the class's minimum first in canonical order -- the longest --
 *      or none when uncovered symbols are strictly cheaper (choice[]), and where its class begins.
 *   e. the backtrack per group from its last record: mark the class's choice (mark[i] bit 1) and go
 *      on at its prev; where the class chose none, at the class in front.
 *      d and e have two forms.  segment_lane_kernel: a lane per group, grid-stride, everything in
 *      scratch -- text whose words are separated by symbols no keyword holds is many small groups.
 *      segment_wave_kernel: a group of K.long_min records or more goes to a wave of its own; the
 *      lanes stage a_i = gap * (end_i - end_{i-1}), b_i = W_i - V[prev] and prev (i) of a chunk into
 *      LDS, V of the last SEGMENT_RING records sits in an LDS ring, one lane takes the dependent
 *      steps at LDS latency and falls back to the scratch copy of V when prev reaches behind the
 *      ring.  No record set is refused: one group of millions of records is slow and correct.
 *   f. the exclusive sum over the tiles' marked records and segment_place_kernel<true>: a stable
 *      compaction into `out`, written from the keyed copies in scratch, so `out` may be the input.
 *      The sums are integer atomics and so deterministic; segment_finish_kernel writes *d_count and
 *      d_sums.
 * Launch geometry never depends on the number of records: capped grids, grid-stride loops. */
constexpr uint32_t SEGMENT_THREADS = 256;
static_assert (SEGMENT_THREADS == CONTEXT_THREADS && SEGMENT_THREADS == SELECT_THREADS, "context_block_scan and select_key_kernel are shared");
constexpr uint32_t SEGMENT_TILE_DEFAULT = 1024, SEGMENT_TILE_MIN = 64, SEGMENT_TILE_MAX = 1u << 20; /* records */
constexpr uint32_t SEGMENT_LONG_DEFAULT = 256, SEGMENT_LONG_MIN = 1, SEGMENT_LONG_MAX = 1u << 30;  /* records of a group */
constexpr uint32_t SEGMENT_CHUNK = 256; /* records a wave stages at a time */
constexpr uint32_t SEGMENT_RING = 512;  /* V of so many records in front stays in LDS */
static_assert ((SEGMENT_RING & (SEGMENT_RING - 1)) == 0 && SEGMENT_CHUNK % WAVE == 0, "ring slots by a mask; whole waves stage");
constexpr uint32_t SEGMENT_COST_LIMIT = 1u << 24;
constexpr uint32_t SEGMENT_BEGINS = 1, SEGMENT_TAKEN = 2; /* mark[] */

/* control words behind SelectCtl, cleared in front of every call */
struct SegmentCtl {
  unsigned long long sums[2]; /* cost and length of the emitted records */
  unsigned int fatal;         /* a keyword_id or a cost out of range: nothing is selected */
  unsigned int n_long;        /* groups in long_list */
};

struct SegmentK {
  SelectK S; /* in, capacity, n_dev, pos_lo, span, lmax, keyed, ctl, error: pass a is SELECT's */
  const uint32_t *cost;
  uint64_t n_keywords;
  uint32_t gap;
  uint32_t tile;                 /* records per tile, a multiple of WAVE */
  uint32_t long_min;             /* groups of so many records take the wave form */
  uint64_t n_tiles;              /* tiles of `capacity` records */
  unsigned long long *tile_min;  /* [n_tiles + 1] minimum start per tile; behind the carry: from the tile on ([n_tiles] stays NEVER) */
  uint32_t *tile_count;          /* [n_tiles + 1] begins (b), then taken records (f) per tile */
  const uint32_t *tile_begin;    /* [n_tiles + 1] the exclusive prefix sum: [n_tiles] = the sum of all */
  uint32_t *mark;                /* [capacity] SEGMENT_BEGINS | SEGMENT_TAKEN */
  uint32_t *group_first;         /* [capacity] */
  uint32_t *prev;                /* [capacity] */
  unsigned long long *V;         /* [capacity] */
  uint32_t *choice, *cfirst;     /* [capacity] */
  uint32_t *long_list;           /* [capacity] */
  ACMRecord *out;
  unsigned long long *d_count, *d_sums;
  SegmentCtl *ctl;
};

/* the records the passes work on */
__device__ __forceinline__ uint64_t
segment_n (const SegmentK &K) {
  return K.ctl->fatal ? 0 : K.S.ctl->n;
}

/* the groups there are: the tiles' prefix sum ends with it (never more than the records) */
__device__ __forceinline__ uint64_t
segment_n_groups (const SegmentK &K) {
  const uint64_t g = K.tile_begin[K.n_tiles];
  return K.ctl->fatal || g > K.S.capacity ? 0 : g;
}

__device__ __forceinline__ uint4
segment_load (const SegmentK &K, uint64_t i) {
  return *reinterpret_cast<const uint4 *> (&K.S.keyed[i]);
}

__device__ __forceinline__ unsigned long long
segment_start (const uint4 r) {
  return ((unsigned long long)r.y << 32) | r.x;
}

__device__ __forceinline__ unsigned long long
segment_end (const uint4 r) {
  return segment_start (r) + r.z - 1;
}

/* pass a, behind SELECT's: the keyword ids against the table's size, the table against the limit.
 * No cost is read through a keyword_id here. */
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_check_kernel (SegmentK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = K.S.ctl->n;
  bool bad = false;
  for (uint64_t i = me; i < n; i += stride)
    bad = bad || K.S.keyed[i].keyword_id >= K.n_keywords;
  for (uint64_t k = me; k < K.n_keywords; k += stride)
    bad = bad || K.cost[k] >= SEGMENT_COST_LIMIT;
  if (bad) {
    K.ctl->fatal = 1;
    if (K.S.error)
      *K.S.error = 1;
  }
}

/* pass b: the tiles' minimum starts */
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_min_kernel (SegmentK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  const uint64_t n = segment_n (K);
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    unsigned long long mn = CONTEXT_NEVER, all;
    if (tile < K.n_tiles && base < n) { /* (uniform in the block; the carry reads every entry) */
      const uint64_t end = base + K.tile < n ? base + K.tile : n;
      for (uint64_t i = base + threadIdx.x; i < end; i += SEGMENT_THREADS) {
        const unsigned long long s = K.S.keyed[i].end_pos; /* (the field holds the start) */
        mn = s < mn ? s : mn;
      }
    }
    (void)context_block_scan<CONTEXT_MIN> (mn, wave_val, all);
    if (threadIdx.x == 0)
      K.tile_min[tile] = all;
  }
}

/* one block: tile_min[i] = the minimum over the tiles from i on, in place (context_carry_kernel's second half) */
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_carry_kernel (SegmentK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  unsigned long long carry = CONTEXT_NEVER, all;
  for (uint64_t base = 0; base < K.n_tiles; base += SEGMENT_THREADS) { /* thread order is descending tile order */
    const bool in = base + threadIdx.x < K.n_tiles;
    const uint64_t i = K.n_tiles - 1 - (base + threadIdx.x);
    const unsigned long long v = in ? K.tile_min[i] : CONTEXT_NEVER;
    const unsigned long long front = context_block_scan<CONTEXT_MIN> (v, wave_val, all);
    if (in)
      K.tile_min[i] = context_op<CONTEXT_MIN> (carry, context_op<CONTEXT_MIN> (front, v));
    carry = context_op<CONTEXT_MIN> (carry, all);
  }
}

/* the begins of the groups: mark[i] and the tile's count */
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_flag_kernel (SegmentK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  const uint64_t n = segment_n (K);
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    unsigned long long cnt = 0, all;
    if (tile < K.n_tiles && base < n) { /* (uniform in the block; the sum behind reads every entry) */
      const uint64_t end = base + K.tile < n ? base + K.tile : n;
      const uint64_t steps = (end - base + SEGMENT_THREADS - 1) / SEGMENT_THREADS;
      unsigned long long carry = K.tile_min[tile + 1]; /* backwards: thread order is descending record order */
      for (uint64_t k = steps; k-- > 0;) {
        const uint64_t i = base + k * SEGMENT_THREADS + (SEGMENT_THREADS - 1 - threadIdx.x);
        const unsigned long long v = i < end ? K.S.keyed[i].end_pos : CONTEXT_NEVER;
        const unsigned long long front = context_block_scan<CONTEXT_MIN> (v, wave_val, all);
        if (i < end) {
          const unsigned long long low = context_op<CONTEXT_MIN> (carry, context_op<CONTEXT_MIN> (front, v));
          const bool begins = i == 0 || low > segment_end (segment_load (K, i - 1));
          K.mark[i] = begins ? SEGMENT_BEGINS : 0u;
          cnt += begins ? 1u : 0u;
        }
        carry = context_op<CONTEXT_MIN> (carry, all);
      }
    }
    (void)context_block_scan<CONTEXT_ADD> (cnt, wave_val, all);
    if (threadIdx.x == 0)
      K.tile_count[tile] = (uint32_t)all;
  }
}

/* pass f's count: the taken records per tile */
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_count_kernel (SegmentK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  const uint64_t n = segment_n (K);
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    unsigned long long cnt = 0, all;
    if (tile < K.n_tiles && base < n) {
      const uint64_t end = base + K.tile < n ? base + K.tile : n;
      for (uint64_t i = base + threadIdx.x; i < end; i += SEGMENT_THREADS)
        cnt += K.mark[i] & SEGMENT_TAKEN ? 1u : 0u;
    }
    (void)context_block_scan<CONTEXT_ADD> (cnt, wave_val, all);
    if (threadIdx.x == 0)
      K.tile_count[tile] = (uint32_t)all;
  }
}

/* behind the prefix sum over the tiles.  EMIT = false: group_first[] (pass b); true: the taken
 * records into `out`, from the keyed copies, and the sums (pass f) */
template <bool EMIT>
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_place_kernel (SegmentK K) {
  __shared__ unsigned long long wave_val[CONTEXT_WAVES];
  const uint64_t n = segment_n (K);
  unsigned long long sum_cost = 0, sum_len = 0, all;
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) */
      break;
    const uint64_t end = base + K.tile < n ? base + K.tile : n;
    uint64_t at = K.tile_begin[tile];
    for (uint64_t step = base; step < end; step += SEGMENT_THREADS) { /* (uniform in the block) */
      const uint64_t i = step + threadIdx.x;
      const bool flag = i < end && (K.mark[i] & (EMIT ? SEGMENT_TAKEN : SEGMENT_BEGINS)) != 0;
      const uint64_t slot = at + context_block_scan<CONTEXT_ADD> (flag ? 1ull : 0ull, wave_val, all);
      at += all;
      if (!flag || slot >= K.S.capacity) /* (the counts add up to at most n) */
        continue;
      if (!EMIT)
        K.group_first[slot] = (uint32_t)i;
      else {
        const uint4 r = segment_load (K, i);
        *reinterpret_cast<uint4 *> (&K.out[slot]) = select_record (r);
        sum_cost += K.cost[r.w]; /* (checked: pass a) */
        sum_len += r.z;
      }
    }
  }
  if (EMIT) {
    (void)context_block_scan<CONTEXT_ADD> (sum_cost, wave_val, all);
    if (threadIdx.x == 0 && all)
      atomicAdd (&K.ctl->sums[0], all);
    (void)context_block_scan<CONTEXT_ADD> (sum_len, wave_val, all);
    if (threadIdx.x == 0 && all)
      atomicAdd (&K.ctl->sums[1], all);
  }
}

/* pass c: prev (i), NONE when no record ends in front of start_i; mark[] is made by pass b */
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_link_kernel (SegmentK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = segment_n (K);
  for (uint64_t i = me; i < n; i += stride) {
    const unsigned long long start = K.S.keyed[i].end_pos; /* (the field holds the start) */
    /* the records in front of lo end in front of start, those from hi on (below i) do not */
    uint64_t lo = 0, hi = i, step = 1;
    while (hi > 0) { /* the gallop: the link is near in canonical order */
      const uint64_t probe = hi > step ? hi - step : 0;
      if (segment_end (segment_load (K, probe)) < start) {
        lo = probe + 1;
        break;
      }
      hi = probe;
      step *= 2;
    }
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (segment_end (segment_load (K, mid)) < start)
        lo = mid + 1;
      else
        hi = mid;
    }
    K.prev[i] = lo ? (uint32_t)(lo - 1) : NONE;
  }
}

/* a group: records [first, last), base = the cut in front (any position at or below its starts
 * and behind every end in front of it) */
__device__ __forceinline__ void
segment_group (const SegmentK &K, uint64_t g, uint64_t n_groups, uint64_t n, uint32_t &first, uint32_t &last, unsigned long long &base) {
  first = K.group_first[g];
  last = g + 1 < n_groups ? K.group_first[g + 1] : (uint32_t)n;
  base = first ? segment_end (segment_load (K, first - 1)) + 1 : K.S.pos_lo;
}

/* the state of pass d between two records of a group */
struct SegmentRun {
  unsigned long long v_last;   /* V of the record in front (0 at the base) */
  unsigned long long gap_path; /* the class's value when its last symbol stays uncovered */
  unsigned long long best_w;   /* the least W of the class so far */
  uint32_t best_i, best_len, best_kw, cls_first;
};

/* one step of pass d: record i with a = gap * (end_i - end of the record in front, or base - 1) and
 * w = W_i.  V, choice and cfirst of EVERY record are written, so that the backtrack reads nothing
 * unwritten whatever the records hold.  Returns V_i. */
__device__ __forceinline__ unsigned long long
segment_step (const SegmentK &K, SegmentRun &R, uint32_t i, bool new_class, unsigned long long a, unsigned long long w, uint32_t len, uint32_t kw) {
  if (new_class) {
    R.gap_path = R.v_last + a;
    R.best_w = ~0ull;
    R.best_i = NONE;
    R.cls_first = i;
  }
  if (R.best_i == NONE || w < R.best_w || (w == R.best_w && (len > R.best_len || (len == R.best_len && kw < R.best_kw)))) { /* at a tie the longest */
    R.best_w = w;
    R.best_i = i;
    R.best_len = len;
    R.best_kw = kw;
  }
  const bool covered = R.best_w <= R.gap_path; /* a keyword wins a tie against uncovered symbols */
  const unsigned long long v = covered ? R.best_w : R.gap_path;
  K.V[i] = v;
  K.choice[i] = covered ? R.best_i : NONE;
  K.cfirst[i] = R.cls_first;
  R.v_last = v;
  return v;
}

/* pass e: one lane, through scratch.  The index falls at every step. */
__device__ __forceinline__ void
segment_backtrack (const SegmentK &K, uint32_t first, uint32_t last) {
  uint32_t at = last - 1;
  while (true) {
    const uint32_t c = K.choice[at];
    uint32_t next;
    if (c != NONE && c <= at && c >= first) {
      K.mark[c] |= SEGMENT_TAKEN;
      next = K.prev[c]; /* below c; NONE: no record in front */
    } else {
      const uint32_t cf = K.cfirst[at];
      next = cf <= at && cf > first ? cf - 1 : NONE;
    }
    if (next == NONE || next < first || next >= at)
      return;
    at = next;
  }
}

/* passes d and e, a lane per group; the long groups are listed for segment_wave_kernel */
__global__ __launch_bounds__ (SEGMENT_THREADS) void
segment_lane_kernel (SegmentK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = segment_n (K), n_groups = segment_n_groups (K);
  for (uint64_t g = me; g < n_groups; g += stride) {
    uint32_t first, last;
    unsigned long long base;
    segment_group (K, g, n_groups, n, first, last, base);
    if (last <= first || last > n) /* never: the begins ascend */
      continue;
    if (last - first >= K.long_min) {
      const uint32_t slot = atomicAdd (&K.ctl->n_long, 1u);
      if (slot < K.S.capacity)
        K.long_list[slot] = (uint32_t)g;
      continue;
    }
    SegmentRun R;
    R.v_last = 0;
    unsigned long long end_front = base - 1;
    for (uint32_t i = first; i < last; i++) {
      const uint4 r = segment_load (K, i);
      const unsigned long long start = segment_start (r), end = segment_end (r);
      const uint32_t p = K.prev[i];
      unsigned long long w;
      if (p != NONE && p >= first)
        w = K.V[p] + (unsigned long long)K.gap * (start - segment_end (segment_load (K, p)) - 1);
      else
        w = (unsigned long long)K.gap * (start - base);
      w += K.cost[r.w];
      (void)segment_step (K, R, i, i == first || end != end_front, (unsigned long long)K.gap * (end - end_front), w, r.z, r.w);
      end_front = end;
    }
    segment_backtrack (K, first, last);
  }
}

/* passes d and e, a wave per long group */
__global__ __launch_bounds__ (WAVE) void
segment_wave_kernel (SegmentK K) {
  __shared__ unsigned long long s_a[SEGMENT_CHUNK], s_b[SEGMENT_CHUNK], s_ring[SEGMENT_RING];
  __shared__ uint32_t s_prev[SEGMENT_CHUNK], s_len[SEGMENT_CHUNK], s_kw[SEGMENT_CHUNK], s_new[SEGMENT_CHUNK];
  const uint64_t n = segment_n (K), n_groups = segment_n_groups (K);
  const uint64_t n_long = K.ctl->n_long < K.S.capacity ? K.ctl->n_long : K.S.capacity;
  for (uint64_t q = blockIdx.x; q < n_long && n_groups; q += gridDim.x) {
    const uint64_t g = K.long_list[q];
    uint32_t first, last;
    unsigned long long base;
    if (g >= n_groups) /* never */
      continue;
    segment_group (K, g, n_groups, n, first, last, base);
    if (last <= first || last > n)
      continue;
    SegmentRun R;
    R.v_last = 0;
    for (uint32_t c0 = first; c0 < last; c0 += SEGMENT_CHUNK) { /* (uniform in the wave) */
      const uint32_t cnt = last - c0 < SEGMENT_CHUNK ? last - c0 : SEGMENT_CHUNK;
      for (uint32_t j = threadIdx.x; j < cnt; j += WAVE) { /* independent loads, side by side */
        const uint32_t i = c0 + j;
        const uint4 r = segment_load (K, i);
        const unsigned long long start = segment_start (r), end = segment_end (r);
        const unsigned long long end_front = i == first ? base - 1 : segment_end (segment_load (K, i - 1));
        const uint32_t p = K.prev[i];
        const bool linked = p != NONE && p >= first;
        unsigned long long b = linked ? (unsigned long long)K.gap * (start - segment_end (segment_load (K, p)) - 1) : (unsigned long long)K.gap * (start - base);
        b += K.cost[r.w];
        s_a[j] = (unsigned long long)K.gap * (end - end_front);
        s_b[j] = b;
        s_prev[j] = linked ? p : NONE;
        s_len[j] = r.z;
        s_kw[j] = r.w;
        s_new[j] = i == first || end != end_front ? 1u : 0u;
      }
      __syncthreads ();
      if (threadIdx.x == 0)
        for (uint32_t j = 0; j < cnt; j++) { /* the dependent steps, at LDS latency */
          const uint32_t i = c0 + j, p = s_prev[j];
          unsigned long long w = s_b[j];
          if (p != NONE) /* (p < i) the ring holds V of the SEGMENT_RING records in front of i */
            w += i - p <= SEGMENT_RING ? s_ring[p & (SEGMENT_RING - 1)] : K.V[p];
          s_ring[i & (SEGMENT_RING - 1)] = segment_step (K, R, i, s_new[j] != 0, s_a[j], w, s_len[j], s_kw[j]);
        }
      __syncthreads (); /* (the next chunk goes into the same LDS) */
    }
    if (threadIdx.x == 0)
      segment_backtrack (K, first, last);
  }
}

/* one lane: the count and the sums.  After an overflowing scan *d_count keeps the count that came in. */
__global__ __launch_bounds__ (WAVE) void
segment_finish_kernel (SegmentK K) {
  if (threadIdx.x != 0 || blockIdx.x != 0)
    return;
  if (K.ctl->fatal) { /* nothing else is written */
    *K.d_count = 0;
    return;
  }
  const bool over = K.S.ctl->n_raw > K.S.capacity;
  const unsigned long long taken = K.tile_begin[K.n_tiles];
  *K.d_count = over ? K.S.ctl->n_raw : taken;
  if (K.d_sums) {
    K.d_sums[0] = K.ctl->sums[0];
    K.d_sums[1] = K.ctl->sums[1];
  }
}
