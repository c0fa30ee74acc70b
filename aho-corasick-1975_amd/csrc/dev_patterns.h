/* dev_patterns.h -- keyword patterns with don't-care gaps: PATTERNS of a record set (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * PATTERNS is a function of a record set in canonical order and of offsets[] (no scan kernel touched, no
 * symbol loaded): a pattern is its fragments at fixed distances, and the record of the fragment that
 * ends last -- the pattern's ANCHOR, the term with the greatest offset + length -- ends where the match
 * does.  So every input record is a candidate anchor: a lane takes one record, reads the postings of the
 * record's keyword in the compiled set (an index inverted by anchor keyword, each keyword's postings by L
 * descending, then pattern id ascending) and, per posting, tests the anchor term's length, computes the
 * match's first symbol S, finds the text of S by a bisection of offsets[], tests that the match ends
 * inside that text, and looks every other term up in the records by its key (end_pos, length) -- unique
 * in canonical order -- with a bisection over the whole input; the keyword id decides.
 * Tiles of K.tile records (a multiple of 64), blocks stride over the tiles, a wave takes 64 consecutive
 * records at a time.  Behind offsets_check_kernel (dev_batch.h; offsets[] given: the batch contract, first
 * 0, last n_symbols, non-decreasing, checked in a launch of its own so that no address is formed from an
 * offset the check has not seen):
 *   1. patterns_count_kernel: count[i] = the matches anchored at record i.  A record that breaks the
 *      contract (a position outside [pos_base, pos_base + n_symbols), a start below pos_base, a length
 *      of 0) is skipped and the plan's error flag raised (select's rule).  A wave in which no lane's
 *      keyword has a posting goes on at once (__ballot).
 *   2. a 64-bit exclusive sum (hipCUB) over the capacity + 1 counts: first[].
 *   3. patterns_fill_kernel: the lanes with matches verify again (nothing is kept between the passes but
 *      the count) and store match j of record i at first[i] + j in posting order, one 16-byte store;
 *      slots at or beyond out_capacity are not written.  One lane writes *d_count.
 *   4. patterns_order_kernel: the matches of one record come out by (L descending, pattern id
 *      ascending), but the matches of one END can come from several anchor records -- fragments of
 *      different lengths that end there -- and interleave in L then.  The lane at the first record of a
 *      group of equal end_pos that holds more than one record sorts the group in place (an insertion
 *      sort: a group is a few runs that are in order already).  Lanes of other groups read nothing of
 *      it but its end_pos, which the sort does not change.
 * Every output slot is written by one lane in each pass; no atomics.  Launch geometry never depends on
 * what the records hold: capped grids, grid-stride loops. */
constexpr uint32_t PATTERNS_THREADS = 256;
constexpr uint32_t PATTERNS_TILE_DEFAULT = 4096, PATTERNS_TILE_MIN = 64, PATTERNS_TILE_MAX = 1u << 20; /* records */

/* a term of a pattern other than its anchor: where it ends in front of the pattern's end */
struct PatternOther {
  uint32_t back, length, keyword_id;
};

struct PatternsK : JoinK { /* (count[i]: the matches anchored at record i) */
  /* the compiled set (ACMPatterns) */
  const uint32_t *anchor_ptr; /* [n_keywords + 1] the postings of a keyword */
  const uint4 *post;          /* { pattern id, L, the anchor term's length, unused } */
  const uint32_t *other_ptr;  /* [n_patterns + 1] a pattern's other terms */
  const PatternOther *other;
  uint32_t n_keywords;
};

/* whether the record (end_pos, length, keyword_id) is among in[0 .. n): a bisection for the first record
 * at or behind the key (end_pos ascending, length descending).  Shared with dev_approx.h. */
__device__ __forceinline__ bool
records_have (const ACMRecord *in, uint64_t n, uint64_t end_pos, uint32_t length, uint32_t keyword_id) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint4 r = *reinterpret_cast<const uint4 *> (&in[mid]);
    const uint64_t pos = ((uint64_t)r.y << 32) | r.x;
    if (pos < end_pos || (pos == end_pos && r.z > length))
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo >= n)
    return false;
  const uint4 r = *reinterpret_cast<const uint4 *> (&in[lo]);
  return ((((uint64_t)r.y << 32) | r.x) == end_pos) && r.z == length && r.w == keyword_id;
}

/* whether the pattern of posting q matches with its anchor at a record of `length` symbols that ends at
 * buffer index e (a record that keeps the contract: e < n_symbols) */
__device__ __forceinline__ bool
patterns_match (const PatternsK &K, uint64_t n, uint64_t e, uint32_t length, const uint4 q) {
  if (length != q.z || (uint64_t)q.y - 1 > e) /* another fragment length, or the match would begin in front of the buffer */
    return false;
  if (K.offsets) { /* (uniform; checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols, and there are texts) */
    const uint64_t t = batch_text_of (K.offsets, 0, K.n_texts - 1, e + 1 - q.y);
    if (e >= K.offsets[t + 1]) /* the match would span a cut */
      return false;
  }
  for (uint32_t j = K.other_ptr[q.x]; j < K.other_ptr[q.x + 1]; j++) {
    const PatternOther o = K.other[j]; /* (back <= L - length of the term: the term begins at or behind S) */
    if (!records_have (K.in, n, K.pos_base + e - o.back, o.length, o.keyword_id))
      return false;
  }
  return true;
}

/* pass 1 */
__global__ __launch_bounds__ (PATTERNS_THREADS) void
patterns_count_kernel (PatternsK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  const uint64_t n = n_raw > K.capacity || K.ctl->bad ? 0 : n_raw; /* an overflowing scan left nothing to join */
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    K.ctl->n = n;
    K.count[K.capacity] = 0; /* (the prefix sum reads capacity + 1 entries) */
  }
  bool bad = false;
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += PATTERNS_THREADS) { /* (uniform in the wave) */
      const uint64_t i = i0 + lane;
      uint4 r = make_uint4 (0, 0, 0, 0);
      uint32_t q = 0, q_end = 0;
      if (i < n) {
        r = *reinterpret_cast<const uint4 *> (&K.in[i]);
        join_postings (K, K.anchor_ptr, K.n_keywords, r, q, q_end, bad);
      }
      uint32_t found = 0;
      if (__ballot (q < q_end)) { /* (else: no lane of the wave anchors anything) */
        const uint64_t e = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
        for (; q < q_end; q++)
          found += patterns_match (K, n, e, r.z, K.post[q]);
      }
      if (i < end)
        K.count[i] = found;
    }
  }
  if (bad && K.error)
    *K.error = 1;
}

/* pass 2 */
__global__ __launch_bounds__ (PATTERNS_THREADS) void
patterns_fill_kernel (PatternsK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = K.ctl->n;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_count = K.first[K.capacity];
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) no record here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * WAVE; i0 < end; i0 += PATTERNS_THREADS) {
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
      join_postings (K, K.anchor_ptr, K.n_keywords, r, q, q_end, bad);
      const uint64_t e = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
      for (; q < q_end && at < at_end; q++) { /* (at < at_end always: pass 1 counted the same matches) */
        const uint4 p = K.post[q];
        if (!patterns_match (K, n, e, r.z, p))
          continue;
        if (at < K.out_capacity)
          *reinterpret_cast<uint4 *> (&K.out[at]) = make_uint4 (r.x, r.y, p.y, p.x);
        at++;
      }
    }
  }
}

/* output order inside a group of equal end_pos: a in front of b */
__device__ __forceinline__ bool
patterns_before (const uint4 a, const uint4 b) {
  return a.z > b.z || (a.z == b.z && a.w < b.w);
}

/* pass 3 (CHAINS runs it too: it reads the head alone) */
__global__ __launch_bounds__ (PATTERNS_THREADS) void
patterns_order_kernel (JoinK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long total = K.first[K.capacity];
  if (total > K.out_capacity) /* the output is unspecified */
    return;
  uint4 *out = reinterpret_cast<uint4 *> (K.out);
  for (uint64_t j = me; j < total; j += stride) {
    const uint4 head = out[j];
    if (j > 0) { /* (the record in front may be moving inside its group: its end_pos does not) */
      const uint4 prev = out[j - 1];
      if (prev.x == head.x && prev.y == head.y)
        continue;
    }
    uint64_t m = 1;
    while (j + m < total) {
      const uint4 next = out[j + m];
      if (next.x != head.x || next.y != head.y)
        break;
      m++;
    }
    for (uint64_t a = 1; a < m; a++) {
      const uint4 key = out[j + a];
      uint64_t b = a;
      while (b > 0) {
        const uint4 left = out[j + b - 1];
        if (!patterns_before (key, left))
          break;
        out[j + b] = left;
        b--;
      }
      if (b != a)
        out[j + b] = key;
    }
  }
}
