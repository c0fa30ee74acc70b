/* dev_select.h -- leftmost-longest non-overlapping matches: SELECT of a record set (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * SELECT is a function of the RECORDS alone, so it is the ordered scan of any plan kind (no scan
 * kernel touched) and passes over what that scan found.  The greedy rule is sequential by its
 * wording -- the next record taken depends on where the last one ended -- but it is the orbit of one
 * point under a map that jumps forward by at most lmax distinct starts, and that is what the passes
 * use.  Behind the scan, on its stream, the record count read on the device (dev_order.h, dev_batch.h):
 *   a. select_key_kernel: every record (end_pos, length, keyword_id) becomes (start, length,
 *      keyword_id) in scratch, start = end_pos + 1 - length.  A record that breaks the contract (a
 *      position outside [pos_lo, pos_lo + span), a start below pos_lo, a length of 0 or beyond the
 *      plan's lmax) raises the plan's error flag and is marked; select_drop_kernel, ONE block that
 *      returns at once when nothing was marked (never expected otherwise), squeezes the marked
 *      records out in place.  dev_order.h's bucket order then sorts the keyed records by (start
 *      ascending, length descending): it is the order it always makes, of another first field.
 *   b. select_cand_kernel, twice (COUNT, prefix sum over the tiles, WRITE: batch_filter_kernel's
 *      shape): a record is a CANDIDATE iff it is the first of its start -- the longest there; no
 *      other record of that start can ever be selected.  The candidates C[0 .. n_c) have distinct
 *      ascending starts.  nxt (i) = the first j with C[j].start >= C[i].start + C[i].length, n_c when
 *      there is none; SELECT = the orbit of candidate 0 under nxt.  Starts are distinct integers, so
 *      C[i + k].start >= C[i].start + k and  i < nxt (i) <= i + C[i].length <= i + lmax.
 *   c. select_tile_kernel<MAP>: tiles of T consecutive candidates, T >= lmax.  A block holds the
 *      starts of its tile and of the first lmax candidates behind it in LDS and finds nxt of every
 *      candidate of the tile by a bisection there.  A chain enters a tile at an offset below lmax:
 *      it comes from a candidate i in front of the tile's first one, f, and nxt (i) <= i + lmax <=
 *      f - 1 + lmax.  For the same reason it never jumps over a tile (T >= lmax).  So the tile's part
 *      in ANY chain is known from min (lmax, T) walks: from each of these entry offsets, the offset
 *      at which the chain enters the next tile and the number of candidates it visits here -- the
 *      tile's entry-to-exit map, a word per offset.
 *   d. select_resolve_kernel, one block: runs the maps from tile 0, offset 0.  The maps of a run of
 *      tiles are loaded by all lanes (coalesced) into LDS, one lane takes the n_c / T dependent
 *      steps there -- LDS latency each, never a global load --, all lanes write the tiles' entry
 *      offsets and output bases.  The total goes to *d_count.  (The maps compose: a prefix scan
 *      under composition would take the serial part away altogether)
 *   e. select_tile_kernel<EMIT>: every tile walks once more from its entry, one lane lists the
 *      visited candidates in LDS, all lanes turn them back into (end_pos, length, keyword_id) at
 *      out[base + j].  The output is written from the candidates in scratch only, so `out` may be
 *      the input array.
 *   f. select_walk_kernel, the general form (lmax > T, or ACM_GPU_SELECT=walk): one lane follows nxt
 *      through global memory, a bisection of dependent loads per selected record.  Slow, correct
 *      for every lmax; the feature refuses no plan.
 * Launch geometry never depends on the number of records: capped grids, grid-stride loops. */
constexpr uint32_t SELECT_THREADS = 256, SELECT_PER = 4, SELECT_CHUNK = SELECT_THREADS * SELECT_PER;
constexpr uint32_t SELECT_WAVES = SELECT_THREADS / WAVE;
constexpr uint32_t SELECT_TILE_DEFAULT = 1024, SELECT_TILE_MIN = 8, SELECT_TILE_MAX = 2048;
constexpr uint32_t SELECT_STAGE = 4096; /* map words the resolve kernel holds in LDS at a time */
static_assert (SELECT_TILE_MAX <= SELECT_STAGE && SELECT_TILE_MAX < (1u << 15), "a tile's map fits the stage; offsets and counts fit 16 bits");
/* LDS of select_tile_kernel: starts of T + E candidates (E <= T), nxt and the list of a tile */
__host__ __device__ constexpr size_t
select_tile_lds (uint32_t T) {
  return (size_t)T * (2 * 8 + 4 + 4);
}
static_assert (select_tile_lds (SELECT_TILE_MAX) <= 64 * 1024, "a tile fits the default LDS limit");

/* control words at the head of the pass's scratch, cleared in front of every call */
struct SelectCtl {
  unsigned long long n;     /* records the passes work on: the input's without the dropped (0 after an overflow) */
  unsigned long long n_raw; /* the count as it came in: what *d_count keeps after an overflow */
  unsigned int n_bad;       /* records that break the contract */
  unsigned int pad[3];
};

struct SelectK {
  const ACMRecord *in;             /* canonical order */
  uint64_t capacity;               /* of `in`, `out` and every scratch array; the count itself when n_dev is NULL */
  const unsigned long long *n_dev; /* the record count (device), or NULL */
  uint64_t pos_lo, span;
  uint32_t lmax;                   /* the larger of the plan's and its delta's */
  uint32_t T, E;                   /* candidates per tile; E = min (lmax, T) entry offsets */
  ACMRecord *keyed;                /* [capacity] (start, length, keyword_id) */
  uint32_t *chunk_count;           /* [n_chunks + 1] candidates per chunk of SELECT_CHUNK keyed records */
  const uint32_t *chunk_begin;     /* [n_chunks + 1] their exclusive prefix sum: [n_chunks] = n_c */
  uint64_t n_chunks;
  ACMRecord *cand;                 /* [capacity] the candidates */
  uint32_t *map;                   /* [tile][E]: exit offset | visited << 16 */
  uint32_t *tile_entry, *tile_base;
  uint64_t max_tiles;              /* tiles of `capacity` candidates */
  ACMRecord *out;
  unsigned long long *d_count;
  SelectCtl *ctl;
  unsigned int *error;             /* the plan's device-side flag (acm_gpu_plan_status) */
};

__global__ __launch_bounds__ (SELECT_THREADS) void
select_key_kernel (SelectK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long n_raw = K.n_dev ? *K.n_dev : K.capacity;
  const uint64_t n = n_raw > K.capacity ? 0 : n_raw; /* an overflowing scan left nothing to select from */
  if (me == 0) {
    K.ctl->n = n;
    K.ctl->n_raw = n_raw;
  }
  uint32_t bad = 0;
  for (uint64_t i = me; i < n; i += stride) {
    uint4 r = *reinterpret_cast<const uint4 *> (&K.in[i]);
    const uint64_t pos = ((uint64_t)r.y << 32) | r.x;
    if (pos < K.pos_lo || pos - K.pos_lo >= K.span || r.z == 0 || r.z > K.lmax || (uint64_t)r.z - 1 > pos - K.pos_lo) {
      r.z = 0; /* marked: select_drop_kernel takes it out */
      bad++;
    } else {
      const uint64_t start = pos + 1 - r.z;
      r.x = (uint32_t)start;
      r.y = (uint32_t)(start >> 32);
    }
    *reinterpret_cast<uint4 *> (&K.keyed[i]) = r;
  }
  if (bad) {
    atomicAdd (&K.ctl->n_bad, bad);
    if (K.error)
      *K.error = 1;
  }
}

/* one block: the marked records out of keyed[0 .. n), in place, order kept.  Chunk by chunk from the
 * front: a chunk is in registers before anything of it is overwritten, and what is written lies at
 * or in front of what was read. */
__global__ __launch_bounds__ (SELECT_THREADS) void
select_drop_kernel (SelectK K) {
  __shared__ uint32_t kept[SELECT_WAVES];
  if (K.ctl->n_bad == 0) /* (uniform) the expected case */
    return;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = K.ctl->n;
  uint64_t at = 0;
  for (uint64_t base = 0; base < n; base += SELECT_THREADS) {
    const uint64_t i = base + threadIdx.x;
    uint4 r = make_uint4 (0, 0, 0, 0);
    if (i < n)
      r = *reinterpret_cast<const uint4 *> (&K.keyed[i]);
    const bool keep = i < n && r.z != 0;
    const uint64_t m = __ballot (keep);
    if (lane == 0)
      kept[wave] = (uint32_t)__popcll (m);
    __syncthreads (); /* (every load of the chunk has been made) */
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < (int)SELECT_WAVES; w++) {
      before += w < (int)wave ? kept[w] : 0u;
      total += kept[w];
    }
    if (keep)
      *reinterpret_cast<uint4 *> (&K.keyed[at + before + rank_below (m)]) = r;
    at += total;
    __syncthreads ();
  }
  if (threadIdx.x == 0)
    K.ctl->n = at;
}

template <bool WRITE>
__global__ __launch_bounds__ (SELECT_THREADS) void
select_cand_kernel (SelectK K) {
  __shared__ uint32_t kept[SELECT_PER * SELECT_WAVES];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const uint64_t n = K.ctl->n;
  for (uint64_t chunk = blockIdx.x; chunk <= K.n_chunks; chunk += gridDim.x) {
    const uint64_t base = chunk * SELECT_CHUNK;
    if (base >= n || chunk == K.n_chunks) { /* (uniform in the block) nothing here: the prefix sum still reads the entry */
      if (!WRITE && threadIdx.x == 0)
        K.chunk_count[chunk] = 0;
      continue;
    }
    uint4 rec[SELECT_PER];
    uint32_t rank[SELECT_PER];
    bool keep[SELECT_PER];
#pragma unroll
    for (int q = 0; q < (int)SELECT_PER; q++) {
      const uint64_t i = base + (uint64_t)q * SELECT_THREADS + threadIdx.x;
      keep[q] = false;
      if (i < n) {
        rec[q] = *reinterpret_cast<const uint4 *> (&K.keyed[i]);
        /* the first of its start (the neighbour's word comes from the cache line a lane beside this one loads) */
        keep[q] = i == 0 || K.keyed[i - 1].end_pos != (((uint64_t)rec[q].y << 32) | rec[q].x);
      }
      const uint64_t m = __ballot (keep[q]);
      rank[q] = rank_below (m);
      if (lane == 0)
        kept[q * SELECT_WAVES + wave] = (uint32_t)__popcll (m);
    }
    __syncthreads ();
    if (!WRITE) {
      if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < (int)(SELECT_PER * SELECT_WAVES); j++)
          total += kept[j];
        K.chunk_count[chunk] = total;
      }
    } else {
      const uint64_t begin = K.chunk_begin[chunk];
#pragma unroll
      for (int q = 0; q < (int)SELECT_PER; q++) {
        uint32_t before = 0;
#pragma unroll
        for (int j = 0; j < (int)(SELECT_PER * SELECT_WAVES); j++)
          before += j < q * (int)SELECT_WAVES + (int)wave ? kept[j] : 0u;
        if (keep[q])
          *reinterpret_cast<uint4 *> (&K.cand[begin + before + rank[q]]) = rec[q];
      }
    }
    __syncthreads (); /* (the next chunk's counts go into the same words) */
  }
}

/* the candidates there are: the chunks' prefix sum ends with it (never more than the records) */
__device__ __forceinline__ uint64_t
select_n_cand (const SelectK &K) {
  const uint64_t n_c = K.chunk_begin[K.n_chunks];
  return n_c > K.capacity ? 0 : n_c;
}

/* a record of the output from a candidate */
__device__ __forceinline__ uint4
select_record (uint4 c) {
  const uint64_t end = (((uint64_t)c.y << 32) | c.x) + c.z - 1;
  return make_uint4 ((uint32_t)end, (uint32_t)(end >> 32), c.z, c.w);
}

/* EMIT = false: the tile's entry-to-exit map (pass c); true: its selected records (pass e).
 * Dynamic LDS: select_tile_lds (T). */
template <bool EMIT>
__global__ __launch_bounds__ (SELECT_THREADS) void
select_tile_kernel (SelectK K) {
  extern __shared__ unsigned long long select_lds[];
  const uint32_t T = K.T, E = K.E;
  unsigned long long *starts = select_lds;                          /* [T + E], the room is 2 T */
  uint32_t *nxt = reinterpret_cast<uint32_t *> (select_lds + 2 * (size_t)T); /* [T] */
  uint32_t *list = nxt + T;                                         /* [T] */
  __shared__ uint32_t s_visited;
  const uint64_t n_c = select_n_cand (K);
  const uint64_t tiles = (n_c + T - 1) / T;
  for (uint64_t tile = blockIdx.x; tile < tiles && tile < K.max_tiles; tile += gridDim.x) {
    const uint64_t first = tile * T;
    const uint32_t here = n_c - first < T ? (uint32_t)(n_c - first) : T; /* candidates of this tile */
    for (uint32_t j = threadIdx.x; j < T + E; j += blockDim.x)
      starts[j] = first + j < n_c ? K.cand[first + j].end_pos : ~0ull; /* (the field holds the start) */
    __syncthreads ();
    for (uint32_t j = threadIdx.x; j < here; j += blockDim.x) {
      const uint32_t len = K.cand[first + j].length;
      const unsigned long long e = starts[j] + len;
      uint32_t lo = j + 1, hi = j + len < T + E - 1 ? j + len : T + E - 1; /* (j + len <= T - 1 + lmax = T + E - 1 by the contract) */
      if (hi < lo)
        hi = lo;
      while (lo < hi) { /* the first entry in (j, j + len] whose start is not below e: the last one is not */
        const uint32_t mid = (lo + hi) / 2;
        if (starts[mid] >= e)
          hi = mid;
        else
          lo = mid + 1;
      }
      nxt[j] = lo;
    }
    __syncthreads ();
    if (!EMIT) {
      for (uint32_t o = threadIdx.x; o < E; o += blockDim.x) {
        uint32_t i = o, visited = 0;
        while (i < here) {
          visited++;
          i = nxt[i];
        }
        uint32_t exit = i >= T ? i - T : 0; /* (a chain that ends in this tile enters no other) */
        if (exit >= E) { /* never, by pass c's argument: no index past a map is ever made */
          exit = E - 1;
          if (K.error)
            *K.error = 1;
        }
        K.map[tile * E + o] = exit | (visited << 16);
      }
    } else {
      if (threadIdx.x == 0) {
        uint32_t i = K.tile_entry[tile], visited = 0;
        while (i < here) {
          list[visited++] = i;
          i = nxt[i];
        }
        s_visited = visited;
      }
      __syncthreads ();
      const uint32_t visited = s_visited;
      const uint64_t base = K.tile_base[tile];
      for (uint32_t j = threadIdx.x; j < visited; j += blockDim.x)
        if (base + j < K.capacity) /* (the bases add up to at most n_c) */
          *reinterpret_cast<uint4 *> (&K.out[base + j]) = select_record (*reinterpret_cast<const uint4 *> (&K.cand[first + list[j]]));
    }
    __syncthreads (); /* (the next tile goes into the same LDS) */
  }
}

/* one block.  After an overflowing scan *d_count keeps the count that came in. */
__global__ __launch_bounds__ (SELECT_THREADS) void
select_resolve_kernel (SelectK K) {
  __shared__ uint32_t stage[SELECT_STAGE];
  __shared__ uint32_t s_entry[SELECT_STAGE], s_base[SELECT_STAGE];
  __shared__ uint32_t s_off, s_sum;
  const uint32_t T = K.T, E = K.E;
  const uint32_t run = SELECT_STAGE / E; /* tiles whose maps the stage holds: at least one */
  const uint64_t n_c = select_n_cand (K);
  const uint64_t tiles = (n_c + T - 1) / T < K.max_tiles ? (n_c + T - 1) / T : K.max_tiles;
  if (threadIdx.x == 0)
    s_off = 0, s_sum = 0;
  __syncthreads ();
  for (uint64_t t0 = 0; t0 < tiles; t0 += run) {
    const uint32_t cnt = tiles - t0 < run ? (uint32_t)(tiles - t0) : run;
    for (uint32_t w = threadIdx.x; w < cnt * E; w += blockDim.x)
      stage[w] = K.map[t0 * E + w];
    __syncthreads ();
    if (threadIdx.x == 0) {
      uint32_t off = s_off, sum = s_sum;
      for (uint32_t g = 0; g < cnt; g++) {
        s_entry[g] = off;
        s_base[g] = sum;
        const uint32_t m = stage[g * E + off];
        sum += m >> 16;
        off = m & 0xFFFFu;
        if (off >= E)
          off = E - 1; /* (select_tile_kernel wrote none such) */
      }
      s_off = off;
      s_sum = sum;
    }
    __syncthreads ();
    for (uint32_t g = threadIdx.x; g < cnt; g += blockDim.x) {
      K.tile_entry[t0 + g] = s_entry[g];
      K.tile_base[t0 + g] = s_base[g];
    }
    __syncthreads ();
  }
  if (threadIdx.x == 0)
    *K.d_count = K.ctl->n_raw > K.capacity ? K.ctl->n_raw : (unsigned long long)s_sum;
}

/* the general form: one lane, nxt through global memory */
__global__ __launch_bounds__ (WAVE) void
select_walk_kernel (SelectK K) {
  if (threadIdx.x != 0 || blockIdx.x != 0)
    return;
  const uint64_t n_c = select_n_cand (K);
  uint64_t i = 0, found = 0;
  while (i < n_c) {
    const uint4 c = *reinterpret_cast<const uint4 *> (&K.cand[i]);
    if (found < K.capacity)
      *reinterpret_cast<uint4 *> (&K.out[found]) = select_record (c);
    found++;
    const uint64_t e = (((uint64_t)c.y << 32) | c.x) + c.z;
    uint64_t lo = i + 1, hi = i + c.z < n_c ? i + c.z : n_c; /* C[i + length].start >= e, or the set ends first */
    if (hi < lo)
      hi = lo;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (K.cand[mid].end_pos >= e)
        hi = mid;
      else
        lo = mid + 1;
    }
    i = lo;
  }
  *K.d_count = K.ctl->n_raw > K.capacity ? K.ctl->n_raw : (unsigned long long)found;
}
