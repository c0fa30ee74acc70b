/* dev_batch.h -- batch scans: many independent texts in one buffer, records per text.
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * Text t of a batch is the symbols [offsets[t], offsets[t + 1]) of one buffer, scanned from the root
 * on its own.  Aho-Corasick reports EVERY occurrence of every keyword, so the matches of text t
 * scanned alone are exactly the matches of the whole buffer that lie entirely inside t: a batch scan
 * is the ordered scan of the concatenation (any plan kind, no scan kernel touched) and one pass
 * over the RECORDS that drops those that begin in an earlier text and says which text each of the
 * others belongs to.  Three kernels behind the scan, on its stream, the record count read on the
 * device as dev_order.h reads it:
 *   1. batch_index_kernel: checks the contract on offsets[] (first 0, last n_symbols, non-
 *      decreasing) and notes, for every block of BATCH_BLOCK = 4,096 positions (dev_order.h's
 *      bucket), the text that holds the block's first position -- a bisection of offsets[] per
 *      block, so that a record's text is searched among the few offsets of one block;
 *   2. batch_filter_kernel, twice: a block takes BATCH_TILE consecutive records of the ordered set,
 *      a lane finds its record's text (index, then a bisection between the index entries of its
 *      block and the next -- neighbouring lanes read the same few offsets) and keeps the record iff
 *      end_pos - length + 1 >= offsets[t].  COUNT: the tile's number of kept records; an exclusive
 *      prefix sum over the tiles (hipCUB) says where each tile's records go; WRITE: the same walk,
 *      rank by ballot within the wave and by the waves' counts in LDS within the block, records and
 *      text ids straight to their final place.  Tiles are consecutive runs of the ordered set and
 *      ranks follow the record index: the compaction is stable, the canonical order survives.
 *      (The ordered set lies in the caller's d_tmp, the kept records go to d_records: no way back.
 *      A single pass with a decoupled look-back would save the second read of the records; the
 *      prefix over tile counts is what dev_order.h and dev_tiles.h already do, and the pass is
 *      proportional to the records, not to the text.)
 *   3. batch_first_kernel: first[t] = number of kept records that end before offsets[t] (one
 *      bisection of the kept records per text: exact for empty texts and for texts without a
 *      match), first[n_texts] = the count, which it also hands to the caller's counter.
 * Launch geometry never depends on the number of texts: grid-stride loops, capped grids. */
constexpr uint32_t BATCH_BLOCK_LOG2 = 12, BATCH_THREADS = 256, BATCH_PER = 4, BATCH_TILE = BATCH_THREADS * BATCH_PER;
constexpr uint32_t BATCH_WAVES = BATCH_THREADS / WAVE;

/* control words at the head of the batch's scratch, cleared in front of every call */
struct BatchCtl {
  unsigned int bad;      /* offsets[] break the contract: no record is reported */
  unsigned int overflow; /* the scan found more records than the buffer holds: *d_count stays the scan's */
  unsigned int pad[2];
};

struct BatchK {
  const ACMRecord *in;             /* the concatenation's records in canonical order */
  uint64_t capacity;               /* of `in` and of `out` */
  const unsigned long long *n_dev; /* the scan's record count (device) */
  const uint64_t *offsets;         /* [n_texts + 1] */
  uint64_t n_texts, n_symbols;
  uint32_t *index;                 /* [n_blocks]: text of position b << BATCH_BLOCK_LOG2 */
  uint64_t n_blocks;               /* (n_symbols >> BATCH_BLOCK_LOG2) + 2 */
  uint32_t *tile_count;            /* [n_tiles + 1] kept records per tile (the last entry stays 0) */
  const uint32_t *tile_begin;      /* [n_tiles + 1] their exclusive prefix sum: [n_tiles] = all kept records */
  uint64_t n_tiles;                /* tiles of `capacity` records */
  ACMRecord *out;
  uint32_t *text_id;               /* may be NULL */
  uint64_t *first;                 /* [n_texts + 1], may be NULL */
  unsigned long long *d_count;
  BatchCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
  /* HEADS instantiations only (flow scans, dev_flows.h): `offsets` are those of an expanded buffer
   * whose text t begins with head[t] symbols carried over from earlier calls.  A record is kept iff
   * it also ends at or behind offsets[t] + head[t]; its end_pos is rebased to base[t], the text's
   * offset in the caller's buffer.  Only the first n_real texts report (what follows is fill), and
   * *pre_bad says that the caller's own checks have failed already. */
  const uint32_t *head;
  const uint64_t *base;            /* [n_real + 1] */
  uint64_t n_real;
  const unsigned int *pre_bad;
};

/* largest t in [lo, hi] with offsets[t] <= pos; offsets[lo] <= pos is the caller's */
__device__ __forceinline__ uint64_t
batch_text_of (const uint64_t *__restrict__ offsets, uint64_t lo, uint64_t hi, uint64_t pos) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] <= pos)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

/* The batch contract on offsets[] (first 0, last n_symbols, non-decreasing) for every family that bisects
 * offsets[] per record -- WORDS, CONTEXT, ANCHORED and the joins (JoinK) --, in a launch of its own so that no
 * address is formed from an offset the check has not seen.  `bad` is the family's control word (cleared by the
 * caller), `error` the plan's flag.  batch_index_kernel's check, without its index. */
constexpr uint32_t OFFSETS_CHECK_THREADS = 256;
__global__ __launch_bounds__ (OFFSETS_CHECK_THREADS) void
offsets_check_kernel (const uint64_t *offsets, uint64_t n_texts, uint64_t n_symbols, unsigned int *bad_word, unsigned int *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (me == 0)
    bad = offsets[0] != 0 || offsets[n_texts] != n_symbols;
  for (uint64_t t = me; t < n_texts; t += stride)
    bad = bad || offsets[t] > offsets[t + 1];
  if (bad) {
    *bad_word = 1;
    if (error)
      *error = 1;
  }
}

template <bool HEADS>
__global__ __launch_bounds__ (BATCH_THREADS) void
batch_index_kernel (BatchK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (me == 0)
    bad = K.offsets[0] != 0 || K.offsets[K.n_texts] != K.n_symbols || (HEADS && *K.pre_bad);
  for (uint64_t t = me; t < K.n_texts; t += stride)
    bad = bad || K.offsets[t] > K.offsets[t + 1];
  if (bad) {
    K.ctl->bad = 1;
    if (K.error)
      *K.error = 1;
  }
  /* (offsets that break the contract still give an index whose entries are texts: what is read
   * through it stays inside offsets[], and nothing of it is reported) */
  for (uint64_t b = me; b < K.n_blocks; b += stride)
    K.index[b] = (uint32_t)batch_text_of (K.offsets, 0, K.n_texts - 1, b << BATCH_BLOCK_LOG2);
}

/* the ordered records of the scan: none when it overflowed (the caller repeats it with room) */
__device__ __forceinline__ uint64_t
batch_n (const BatchK &K) {
  const unsigned long long c = *K.n_dev;
  return c > K.capacity ? 0 : c;
}

template <bool WRITE, bool HEADS>
__global__ __launch_bounds__ (BATCH_THREADS) void
batch_filter_kernel (BatchK K) {
  __shared__ uint32_t kept[BATCH_PER * BATCH_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = batch_n (K);
  if (!WRITE && blockIdx.x == 0 && threadIdx.x == 0)
    K.ctl->overflow = *K.n_dev > K.capacity ? 1u : 0u;
  for (uint64_t tile = blockIdx.x; tile <= K.n_tiles; tile += gridDim.x) {
    const uint64_t base = tile * BATCH_TILE;
    if (base >= n || tile == K.n_tiles) { /* (uniform in the block) nothing here: the prefix sum still reads the entry */
      if (!WRITE && threadIdx.x == 0)
        K.tile_count[tile] = 0;
      continue;
    }
    uint4 rec[BATCH_PER];
    uint32_t tid[BATCH_PER], rank[BATCH_PER];
    bool keep[BATCH_PER];
#pragma unroll
    for (int q = 0; q < (int)BATCH_PER; q++) {
      const uint64_t i = base + (uint64_t)q * BATCH_THREADS + threadIdx.x;
      keep[q] = false;
      tid[q] = 0;
      if (i < n) {
        rec[q] = *reinterpret_cast<const uint4 *> (&K.in[i]);
        const uint64_t pos = ((uint64_t)rec[q].y << 32) | rec[q].x;
        if (pos >= K.n_symbols) { /* not a position of the buffer (never expected): dropped, reported */
          if (K.error)
            *K.error = 1;
        } else {
          const uint64_t b = pos >> BATCH_BLOCK_LOG2;
          uint64_t lo = K.index[b], hi = K.index[b + 1];
          if (hi > K.n_texts - 1)
            hi = K.n_texts - 1;
          if (lo > hi)
            lo = hi;
          const uint64_t t = batch_text_of (K.offsets, lo, hi, pos);
          tid[q] = (uint32_t)t;
          keep[q] = pos + 1 >= K.offsets[t] + rec[q].z; /* the match begins inside its text */
          if (HEADS) {
            const uint64_t body = K.offsets[t] + (t < K.n_real ? K.head[t] : 0); /* (read in bounds also when nothing is kept) */
            keep[q] = keep[q] && t < K.n_real && pos >= body;
            const uint64_t at = pos - body + (t < K.n_real ? K.base[t] : 0);
            rec[q].x = (uint32_t)at;
            rec[q].y = (uint32_t)(at >> 32);
          }
        }
      }
      const uint64_t m = __ballot (keep[q]);
      rank[q] = rank_below (m);
      if (lane == 0)
        kept[q * BATCH_WAVES + wave] = (uint32_t)__popcll (m);
    }
    __syncthreads ();
    if (!WRITE) {
      if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < (int)(BATCH_PER * BATCH_WAVES); j++)
          total += kept[j];
        K.tile_count[tile] = total;
      }
    } else {
      /* index order within the tile is (q, wave, lane): the kept records in front of this lane's */
      const uint64_t begin = K.tile_begin[tile];
#pragma unroll
      for (int q = 0; q < (int)BATCH_PER; q++) {
        uint32_t before = 0;
#pragma unroll
        for (int j = 0; j < (int)(BATCH_PER * BATCH_WAVES); j++)
          before += j < q * (int)BATCH_WAVES + (int)wave ? kept[j] : 0u;
        if (keep[q]) {
          const uint64_t at = begin + before + rank[q];
          *reinterpret_cast<uint4 *> (&K.out[at]) = rec[q];
          if (K.text_id)
            K.text_id[at] = tid[q];
        }
      }
    }
    __syncthreads (); /* (the next tile's counts go into the same words) */
  }
}

template <bool HEADS>
__global__ __launch_bounds__ (BATCH_THREADS) void
batch_first_kernel (BatchK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool overflow = K.ctl->overflow != 0;
  const uint64_t n = K.ctl->bad || overflow ? 0 : K.tile_begin[K.n_tiles];
  if (me == 0 && (!overflow || (HEADS && K.ctl->bad))) /* (a bad flow call has scanned fill: whatever that found, nothing is reported) */
    *K.d_count = n;
  if (!K.first)
    return;
  const uint64_t n_texts = HEADS ? K.n_real : K.n_texts;
  for (uint64_t t = me; t <= n_texts; t += stride) {
    const uint64_t off = HEADS ? (K.ctl->bad ? 0 : K.base[t]) : K.offsets[t];
    uint64_t lo = 0, hi = n; /* the first kept record that ends at or behind offsets[t] */
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (K.out[mid].end_pos < off)
        lo = mid + 1;
      else
        hi = mid;
    }
    K.first[t] = t == n_texts ? n : lo;
  }
}
