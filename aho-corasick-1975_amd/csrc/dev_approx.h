/* dev_approx.h -- keywords with up to k mismatches: APPROX of a record set (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * A target of L symbols with budget k is cut into k + 1 pieces; the pieces are the dictionary, and every
 * exact record of a piece is a SEED: it says where its target would begin (S = end + 1 - length - offset),
 * and the target is verified against the caller's text there.  The compiled set (ACMApprox) is an index
 * inverted by term keyword -- a keyword's postings (target id, term index j, offset, term length) sorted by
 * (target id, j) --, per target (L, k, its first term), the terms, and the spellings in the caller's symbols.
 * One GROUP of 16 consecutive lanes takes one input record, so a wave takes four records at a time; tiles of
 * K.tile records (a multiple of 64), blocks stride over the tiles.  Behind offsets_check_kernel (dev_batch.h;
 * offsets[] given: the batch contract, checked in a launch of its own so that no address is formed from an offset
 * the check has not seen):
 *   1. approx_count_kernel: count[i] = the matches seeded by record i.  Per posting the group runs the cheap
 *      tests (all 16 lanes the same: the term's length is the record's, S >= 0, the text of S by a bisection
 *      of offsets[], S + L ends inside that text).  Then the group verifies: lane j compares symbols j,
 *      j + 16, ... of target and text, naturally aligned loads of one symbol, consecutive lanes on
 *      consecutive symbols; after each round the group's mismatches grow by the popcount of its 16 bits of
 *      the wave's __ballot, and the group stops once they exceed k.  The round loop is wave-uniform: it runs
 *      to the longest of the wave's four candidates with finished groups predicated off, so every __ballot
 *      is executed by all 64 lanes.  A candidate within its budget is dropped when a term of lower index of
 *      the same target has its record in the input too (records_have of dev_patterns.h, a bisection of the
 *      whole input): that term's group emits the match, so a match comes out once however many pieces seed
 *      it.  This test stands behind the verification because it is the dear one -- some twenty dependent
 *      loads -- and few candidates get that far (DESIGN.md 4.23 has both orders measured).
 *      A wave in which no record has a posting goes on at once.
 *      A record that breaks the contract is skipped and the plan's error flag raised (select's rule).
 *   2. a 64-bit exclusive sum (hipCUB) over the capacity + 1 counts: first[].
 *   3. approx_fill_kernel: the groups with a nonzero count verify again (nothing is kept between the passes
 *      but the count) and lane 0 of the group stores match j of record i at first[i] + j of the call's
 *      scratch, one 16-byte store plus its distance; slots at or beyond out_capacity are not written.
 *   4. the order, only when the total fits out_capacity: the seeds lie anywhere inside their targets, so the
 *      fill order is not the output order.  approx_key1_kernel, a stable radix sort (hipCUB) of an index
 *      permutation by (longest - length, target id), approx_key2_kernel, a second stable sort by end_pos -
 *      pos_base, approx_gather_kernel: records and distances to d_out and d_dist.
 * Every slot is written by one lane in each pass; no atomics.  Launch geometry never depends on what the
 * records hold: capped grids, grid-stride loops. */
constexpr uint32_t APPROX_THREADS = 256, APPROX_GROUP = 16, APPROX_PER_WAVE = WAVE / APPROX_GROUP, APPROX_PER_BLOCK = APPROX_THREADS / APPROX_GROUP;
constexpr uint32_t APPROX_TILE_DEFAULT = 1024, APPROX_TILE_MIN = 64, APPROX_TILE_MAX = 1u << 20; /* records */

/* a term of a target: the piece of `length` symbols at `offset` is keyword keyword_id */
struct ApproxTerm {
  uint32_t offset, length, keyword_id;
};

struct ApproxK : JoinK { /* (count[i]: the matches seeded by record i) */
  /* the compiled set (ACMApprox) */
  const uint32_t *post_ptr;  /* [n_keywords + 1] the postings of a keyword */
  const uint4 *post;         /* { target id, term index j inside the target, the term's offset, the term's length } */
  const uint4 *target;       /* [n_targets] { L, k, the target's first term in terms[], unused } */
  const uint64_t *spell_off; /* [n_targets] the spelling's first symbol in spell[] */
  const ApproxTerm *terms;
  const void *spell; /* the spellings, symbols of the caller's size */
  uint32_t n_keywords;
  uint32_t longest, tgt_bits; /* the longest L; bits of a target id (sort key 1) */
  const void *text;           /* the caller's symbols */
  ACMRecord *fill;            /* [out_capacity] the matches in fill order (scratch) */
  uint32_t *fill_dist;        /* [out_capacity] their distances */
  uint64_t *key;              /* [out_capacity] the sort key a key kernel writes */
  uint32_t *idx, *idx_from;   /* [out_capacity] the permutation a kernel writes / reads */
  uint32_t *dist;             /* beside JoinK::out; may be NULL */
  /* TEMPLATES only (dev_templates.h): the cells beside the spellings and the compiled classes */
  const uint32_t *cells;      /* [the spellings' symbols] ACM_TEMPLATE_LITERAL, ACM_TEMPLATE_ANY or a class id */
  const uint32_t *cls_bitmap; /* 1-byte symbols: [n_classes][8] the accepted symbols, the negate flag applied */
  const uint64_t *cls_ptr;    /* wider symbols: [n_classes + 1] the ranges of a class in cls_ranges ... */
  const void *cls_ranges;     /* ... pairs lo, hi of the caller's size ... */
  const uint32_t *cls_flags;  /* ... and ACM_TEMPLATE_NEGATED */
};

/* What a wave does with its four records: every group walks the postings [q, q_end) of its record r (none: q ==
 * q_end) and returns the number of matches it seeds; with FILL it stores them from slot `at` on.  All 64 lanes
 * call this together; q, q_end, r and `at` are the same in the 16 lanes of a group.  With CELLS the targets are templates: a position
 * is accepted by its cell (templates_cell_fails of dev_templates.h), not by its spelling alone. */
template <typename T>
__device__ __forceinline__ bool templates_cell_fails (const ApproxK &K, uint32_t cell, const T *__restrict__ text_at, const T *__restrict__ spell_at);

template <typename T, bool FILL, bool CELLS>
__device__ __forceinline__ uint32_t
approx_group (const ApproxK &K, uint64_t n, const uint4 r, uint32_t q, uint32_t q_end, unsigned long long at) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), sub = lane & (APPROX_GROUP - 1), shift = lane & ~(APPROX_GROUP - 1);
  const T *__restrict__ text = static_cast<const T *> (K.text);
  const uint64_t e = (((uint64_t)r.y << 32) | r.x) - K.pos_base;
  uint32_t found = 0;
  while (__ballot (q < q_end)) { /* (uniform in the wave) */
    bool cand = false;
    uint32_t L = 0, k = 0, w = 0, lower = 0, lower_end = 0; /* [lower, lower_end): the target's terms of lower index */
    uint64_t S = 0;
    const T *__restrict__ spell = nullptr;
    const uint32_t *__restrict__ cells = nullptr;
    if (q < q_end) {
      const uint4 p = K.post[q++];
      if (r.z == p.w && (uint64_t)p.z + p.w - 1 <= e) { /* the piece's length, and the target begins inside the buffer */
        const uint4 tg = K.target[p.x];
        w = p.x;
        L = tg.x;
        k = tg.y;
        S = e + 1 - p.w - p.z;
        uint64_t t_hi = K.n_symbols;
        if (K.offsets) /* (uniform; checked offsets: 0 = offsets[0] <= ... <= offsets[n_texts] = n_symbols, and there are texts) */
          t_hi = K.offsets[batch_text_of (K.offsets, 0, K.n_texts - 1, S) + 1];
        cand = S + L <= t_hi; /* else: the target would end behind the buffer or span a cut */
        lower = tg.z;
        lower_end = tg.z + p.y;
        spell = static_cast<const T *> (K.spell) + K.spell_off[w];
        if (CELLS)
          cells = K.cells + K.spell_off[w];
      }
    }
    uint32_t miss = 0;
    for (uint32_t i0 = 0;; i0 += APPROX_GROUP) { /* (uniform in the wave: to the longest of its candidates) */
      const bool active = cand && i0 < L && miss <= k;
      if (!__ballot (active))
        break;
      const uint32_t i = i0 + sub;
      bool differ = false;
      if (active && i < L)
        differ = CELLS ? templates_cell_fails<T> (K, cells[i], text + S + i, spell + i) : text[S + i] != spell[i];
      miss += __popcll ((__ballot (differ) >> shift) & 0xFFFFull);
    }
    bool match = cand && miss <= k;
    for (; match && lower < lower_end; lower++) { /* a term of lower index that seeds this match emits it */
      const ApproxTerm o = K.terms[lower];
      match = !records_have (K.in, n, K.pos_base + S + o.offset + o.length - 1, o.length, o.keyword_id);
    }
    if (match) {
      if (FILL) {
        if (sub == 0 && at < K.out_capacity) {
          const uint64_t end_pos = K.pos_base + S + L - 1;
          *reinterpret_cast<uint4 *> (&K.fill[at]) = make_uint4 ((uint32_t)end_pos, (uint32_t)(end_pos >> 32), L, w);
          K.fill_dist[at] = miss;
        }
        at++;
      }
      found++;
    }
  }
  return found;
}

/* pass 1 */
template <typename T, bool CELLS = false>
__global__ __launch_bounds__ (APPROX_THREADS) void
approx_count_kernel (ApproxK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, group = lane / APPROX_GROUP;
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
    for (uint64_t i0 = base + (uint64_t)wave * APPROX_PER_WAVE; i0 < end; i0 += APPROX_PER_BLOCK) { /* (uniform in the wave) */
      const uint64_t i = i0 + group;
      uint4 r = make_uint4 (0, 0, 0, 0);
      uint32_t q = 0, q_end = 0;
      if (i < n) {
        r = *reinterpret_cast<const uint4 *> (&K.in[i]);
        join_postings (K, K.post_ptr, K.n_keywords, r, q, q_end, bad);
      }
      const uint32_t found = approx_group<T, false, CELLS> (K, n, r, q, q_end, 0);
      if (i < end && (lane & (APPROX_GROUP - 1)) == 0)
        K.count[i] = found;
    }
  }
  if (bad && K.error)
    *K.error = 1;
}

/* pass 2 */
template <typename T, bool CELLS = false>
__global__ __launch_bounds__ (APPROX_THREADS) void
approx_fill_kernel (ApproxK K) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, group = lane / APPROX_GROUP;
  const uint64_t n = K.ctl->n;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *K.d_count = K.first[K.capacity];
  for (uint64_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * K.tile;
    if (base >= n) /* (uniform in the block) no record here */
      continue;
    const uint64_t end = base + K.tile < K.capacity ? base + K.tile : K.capacity;
    for (uint64_t i0 = base + (uint64_t)wave * APPROX_PER_WAVE; i0 < end; i0 += APPROX_PER_BLOCK) {
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
      (void)approx_group<T, true, CELLS> (K, n, r, q, q_end, at);
    }
  }
}

/* pass 3: the identity permutation and the first sort's key, (longest - length) above the target id; slots behind
 * the matches get a key above every match's */
__global__ __launch_bounds__ (APPROX_THREADS) void
approx_key1_kernel (ApproxK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long total = K.first[K.capacity];
  if (total > K.out_capacity) /* no output */
    return;
  for (uint64_t j = me; j < K.out_capacity; j += stride) {
    uint64_t key = (uint64_t)K.longest << K.tgt_bits;
    if (j < total) {
      const uint4 m = *reinterpret_cast<const uint4 *> (&K.fill[j]);
      key = ((uint64_t)(K.longest - m.z) << K.tgt_bits) | m.w;
    }
    K.key[j] = key;
    K.idx[j] = (uint32_t)j;
  }
}

/* the second sort's key of the permuted matches: end_pos - pos_base, n_symbols behind the matches */
__global__ __launch_bounds__ (APPROX_THREADS) void
approx_key2_kernel (ApproxK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long total = K.first[K.capacity];
  if (total > K.out_capacity)
    return;
  for (uint64_t j = me; j < K.out_capacity; j += stride) {
    uint64_t key = K.n_symbols;
    const uint32_t from = K.idx_from[j];
    if (j < total && from < total) {
      const uint4 m = *reinterpret_cast<const uint4 *> (&K.fill[from]);
      key = (((uint64_t)m.y << 32) | m.x) - K.pos_base;
    }
    K.key[j] = key;
  }
}

__global__ __launch_bounds__ (APPROX_THREADS) void
approx_gather_kernel (ApproxK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long total = K.first[K.capacity];
  if (total > K.out_capacity)
    return;
  for (uint64_t j = me; j < total; j += stride) {
    const uint32_t from = K.idx_from[j];
    if (from >= total) /* (never: the matches' keys are below the padding's) */
      continue;
    *reinterpret_cast<uint4 *> (&K.out[j]) = *reinterpret_cast<const uint4 *> (&K.fill[from]);
    if (K.dist)
      K.dist[j] = K.fill_dist[from];
  }
}
