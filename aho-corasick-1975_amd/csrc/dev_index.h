/* dev_index.h -- the inverted index of a batch: the transposition of the text x keyword count matrix
 * in CSR form into the postings of every keyword, ascending by text id, and the concatenation of two
 * such indexes (include/acm_index.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The passes of the transposition, all on the caller's stream:
 *   1. rules_check_kernel (dev_rules.h): row_ptr[] begins with 0 and never decreases, or the call
 *      stops (the plan's error flag; no later pass forms an address from a row pointer then).
 *   2. index_hist_kernel: a lane per matrix entry; cnt[k] += 1 for its keyword, first in one of the
 *      block's 2,048 LDS counters (a keyword owns the counter k mod 2,048 when it is the first to ask
 *      for it; another that finds it taken adds to cnt[k] at once), which the block adds to cnt[] at
 *      its end.  Posting lists are as skewed as word counts, and a dictionary sorted by frequency has
 *      its stop-words next to each other: an atomic per entry would meet on a few cache lines.  A
 *      col >= n_keywords is not counted and raises the error flag.
 *   3. An exclusive sum of the counts (hipCUB) in scratch: ptr[].  index_finish_kernel copies it to
 *      d_post_ptr, writes *d_nnz (through scratch, so that a stopped call writes nothing else),
 *      counts the lists of either form, puts the keywords whose lists pass 5 sorts on tier[] -- the
 *      one-wave tier's from the front, the one-block tier's from the back -- and leaves wcnt[k] =
 *      df[k] for the WIDE lists (df above `list`), 0 for the others; a second exclusive sum gives
 *      wbase[], the wide entries in front of keyword k.  A call that only counts, or whose room is
 *      too small, ends here.
 *   4. index_scatter_kernel: a lane per matrix entry again; its text is found by bisection in
 *      row_ptr[].  An entry of a list of the fast form goes to ptr[k] + a slot from the keyword's
 *      counter, counted back down (at most `list` atomics on a word); an entry of a wide list is
 *      appended to the sort room as the key keyword << 31 | t and its count, one atomic per wave.
 *      The room was filled with all-ones keys before: the sentinels behind a fill that only the
 *      device knows.
 *   5. FAST: index_sort_kernel<64, 0> puts every list of 2 to min (list, 256) entries in order, one
 *      wave (a block of 64 lanes) per list; index_sort_kernel<256, 1> those of 257 to `list` entries,
 *      one block per list.  The blocks stride over their tier's part of tier[], so the lists are
 *      spread evenly however the keywords lie: keys text << 32 | slot, bitonic in LDS, the counts
 *      beside them.  Text ids are unique within a list, so whatever order the atomics of pass 4 left
 *      is gone.
 *   6. WIDE: a radix sort (hipCUB) of the sort room by the key's 31 + bits (n_keywords) bits, then
 *      index_wide_put_kernel: the j-th sorted entry, of keyword k, is posting j - wbase[k] of k.  The
 *      sort runs over the whole room whatever it holds, so its launches depend on no count on the
 *      device; one long list costs what many do.  The host leaves pass 6 and its scratch out when
 *      n_texts <= list: no list is longer than the batch has texts.
 * LDS of the fast form: 16 bytes per entry: 4 KiB for the one-wave tier, 16 KiB per block at the
 * default `list` of 1,024, 64 KiB at the largest, 4,096; 16 KiB of counters in pass 2.  Scratch: 20 bytes
 * per keyword (cnt, ptr, tier), 16 more (wcnt, wbase) and 32 bytes per entry of the room with a wide form.
 *
 * CONCAT is entry-parallel: index_concat_check_kernel sees the two pointer arrays, then every
 * list's boundary; index_concat_finish_kernel writes out_ptr[k] = a_ptr[min (k, n_a)] + b_ptr[k];
 * index_concat_fill_kernel finds the keyword of every output entry by bisection over that sum. */
constexpr uint32_t INDEX_LIST_DEFAULT = 1024, INDEX_LIST_MAX = 4096;
constexpr uint32_t INDEX_WAVE_LIST = 256; /* the longest list one wave sorts */
constexpr uint32_t INDEX_SORT_THREADS = 256;
constexpr uint32_t INDEX_HIST_SLOTS = 2048; /* LDS counters of a block of the count pass: 16 KiB */
constexpr uint32_t INDEX_TEXT_BITS = 31; /* n_texts < 2^31 */
static_assert ((INDEX_LIST_MAX & (INDEX_LIST_MAX - 1)) == 0 && (INDEX_WAVE_LIST & (INDEX_WAVE_LIST - 1)) == 0, "the sorts pad to a power of two");

/* control words behind the RulesCtl at the head of the scratch, cleared in front of every call */
struct IndexCtl {
  unsigned long long n_wide; /* entries appended to the sort room */
  unsigned long long forms[2];
  unsigned int n_tier[2]; /* lists on tier[]: the one-wave tier's from the front, the one-block tier's from the back */
};

struct IndexK {
  RulesK G; /* the gate: rules_stopped (G) stops every pass; row_ptr, n_texts, ctl, error and the tally in front */
  const uint32_t *col;
  const unsigned long long *val;
  uint64_t n_keywords, text_base, post_capacity;
  uint32_t list; /* the longest list of the fast form */
  /* scratch */
  IndexCtl *ictl;
  unsigned long long *cnt;         /* [n_keywords + 1] entries per keyword, the last stays 0; counted back down by the scatter */
  const unsigned long long *ptr;   /* [n_keywords + 1] their exclusive sum */
  unsigned long long *wcnt;        /* [n_keywords + 1] df of the wide lists; nullptr: no wide form in this call */
  const unsigned long long *wbase; /* [n_keywords + 1] its exclusive sum */
  uint32_t *tier;                  /* [n_keywords] the keywords whose lists the fast form sorts, by tier (IndexCtl::n_tier) */
  unsigned long long *wkey, *wval; /* [post_capacity] the sort room as the scatter fills it */
  const unsigned long long *skey, *sval; /* the same, sorted */
  /* outputs */
  unsigned long long *d_post_ptr, *d_nnz, *d_forms, *d_post_count;
  uint32_t *d_post_text;
};

/* the entries the fill passes may write: all of them, when they fit */
__device__ __forceinline__ bool
index_fills (const IndexK &K) {
  return K.d_post_text != nullptr && K.ptr[K.n_keywords] <= K.post_capacity;
}

/* pass 2.  INDEX_HIST_SLOTS counters of the block in LDS, one keyword each (the first that asks for the slot k mod
 * INDEX_HIST_SLOTS owns it); a keyword that finds its slot taken adds to the global counter at once. */
__global__ __launch_bounds__ (256) void
index_hist_kernel (IndexK K) {
  __shared__ uint32_t s_key[INDEX_HIST_SLOTS], s_cnt[INDEX_HIST_SLOTS];
  if (rules_stopped (K.G))
    return;
  for (uint32_t i = threadIdx.x; i < INDEX_HIST_SLOTS; i += blockDim.x) {
    s_key[i] = NONE;
    s_cnt[i] = 0;
  }
  __syncthreads ();
  const unsigned long long n = K.G.row_ptr[K.G.n_texts];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const uint32_t k = K.col[e];
    if (k >= K.n_keywords) {
      bad = true;
      continue;
    }
    const uint32_t slot = k & (INDEX_HIST_SLOTS - 1);
    const uint32_t owner = atomicCAS (&s_key[slot], NONE, k);
    if (owner == NONE || owner == k)
      atomicAdd (&s_cnt[slot], 1u); /* (a block strides over fewer than 2^32 entries) */
    else
      atomicAdd (&K.cnt[k], 1ull);
  }
  __syncthreads ();
  for (uint32_t i = threadIdx.x; i < INDEX_HIST_SLOTS; i += blockDim.x)
    if (s_cnt[i])
      atomicAdd (&K.cnt[s_key[i]], (unsigned long long)s_cnt[i]);
  if (bad && K.G.error)
    *K.G.error = 1;
}

/* pass 3, behind the first sum */
__global__ __launch_bounds__ (256) void
index_finish_kernel (IndexK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool stop = rules_stopped (K.G);
  if (me == 0)
    *K.d_nnz = stop ? 0ull : K.ptr[K.n_keywords];
  if (stop) /* every other output stays as it was */
    return;
  const bool fills = index_fills (K);
  unsigned long long fast = 0, wide = 0;
  for (uint64_t k = me; k <= K.n_keywords; k += stride) {
    const unsigned long long at = K.ptr[k], df = k < K.n_keywords ? K.ptr[k + 1] - at : 0ull;
    K.d_post_ptr[k] = at;
    if (K.wcnt)
      K.wcnt[k] = df > K.list ? df : 0ull;
    fast += fills && df >= 1 && df <= K.list;
    wide += fills && df > K.list;
    if (fills && df >= 2 && df <= K.list) { /* a list for pass 5: fewer than n_keywords of them, so the two ends never meet */
      if (df <= INDEX_WAVE_LIST)
        K.tier[atomicAdd (&K.ictl->n_tier[0], 1u)] = (uint32_t)k;
      else
        K.tier[K.n_keywords - 1 - atomicAdd (&K.ictl->n_tier[1], 1u)] = (uint32_t)k;
    }
  }
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    fast += __shfl_xor ((uint32_t)fast, d, WAVE); /* (a lane strides over fewer than 2^32 keywords) */
    wide += __shfl_xor ((uint32_t)wide, d, WAVE);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (fast)
      atomicAdd (&K.ictl->forms[0], fast);
    if (wide)
      atomicAdd (&K.ictl->forms[1], wide);
  }
}

/* the last launch of a call: the two form counters, once every pass has added to them */
__global__ __launch_bounds__ (WAVE) void
index_forms_kernel (IndexK K) {
  if (rules_stopped (K.G) || !K.d_forms || threadIdx.x >= 2)
    return;
  K.d_forms[threadIdx.x] = K.ictl->forms[threadIdx.x];
}

/* pass 4 */
__global__ __launch_bounds__ (256) void
index_scatter_kernel (IndexK K) {
  if (rules_stopped (K.G) || !index_fills (K))
    return;
  const unsigned long long n = K.G.row_ptr[K.G.n_texts];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t first = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); first < n; first += stride) { /* (uniform in the wave) */
    const uint64_t e = first + lane;
    const uint32_t k = e < n ? K.col[e] : 0u;
    const bool ok = e < n && k < K.n_keywords;
    unsigned long long begin = 0, df = 0, v = 0;
    uint64_t t = 0;
    if (ok) {
      begin = K.ptr[k];
      df = K.ptr[k + 1] - begin;
      v = K.val[e];
      /* the text of entry e: the last row that begins at or in front of e (the empty rows in front of it begin there too) */
      uint64_t hi = K.G.n_texts;
      while (t < hi) {
        const uint64_t mid = t + ((hi - t) >> 1);
        if (K.G.row_ptr[mid + 1] <= e)
          t = mid + 1;
        else
          hi = mid;
      }
    }
    const bool wide = ok && K.wkey && df > K.list;
    if (ok && !wide) {
      const unsigned long long left = atomicAdd (&K.cnt[k], ~0ull); /* (minus one) */
      if (left >= 1 && left <= df) { /* (the entries the count pass counted: always) */
        K.d_post_text[begin + left - 1] = (uint32_t)(K.text_base + t);
        K.d_post_count[begin + left - 1] = v;
      }
    }
    const uint64_t m = __ballot (wide);
    if (m) {
      unsigned long long base = 0;
      if ((int)lane == __ffsll ((unsigned long long)m) - 1)
        base = atomicAdd (&K.ictl->n_wide, (unsigned long long)__popcll (m));
      const int leader = __ffsll ((unsigned long long)m) - 1;
      base = ((unsigned long long)__shfl ((uint32_t)(base >> 32), leader, WAVE) << 32) | __shfl ((uint32_t)base, leader, WAVE);
      const unsigned long long slot = base + rank_below (m);
      if (wide && slot < K.post_capacity) { /* (the wide entries are among the nnz that fit: always) */
        K.wkey[slot] = ((unsigned long long)k << INDEX_TEXT_BITS) | t;
        K.wval[slot] = v;
      }
    }
  }
}

/* pass 5: the lists of tier TIER (0: 2 to INDEX_WAVE_LIST entries, 1: more, up to K.list), a block per list; `room`: the
 * longest list of the tier */
template <uint32_t THREADS, uint32_t TIER>
__global__ __launch_bounds__ (THREADS) void
index_sort_kernel (IndexK K, uint32_t room) {
  extern __shared__ unsigned long long index_lds[];
  if (rules_stopped (K.G) || !index_fills (K))
    return;
  uint32_t p2_room = 1;
  while (p2_room < room)
    p2_room <<= 1;
  unsigned long long *key = index_lds, *cntl = index_lds + p2_room;
  const uint32_t me = threadIdx.x, n_lists = K.ictl->n_tier[TIER];
  for (uint32_t l = blockIdx.x; l < n_lists; l += gridDim.x) { /* (uniform in the block) */
    const uint64_t k = TIER ? K.tier[K.n_keywords - 1 - l] : K.tier[l];
    const unsigned long long begin = K.ptr[k], len = K.ptr[k + 1] - begin;
    if (len < 2 || len > room) /* (what pass 3 put on the tier: never) */
      continue;
    const uint32_t df = (uint32_t)len;
    uint32_t p2 = 2;
    while (p2 < df)
      p2 <<= 1;
    for (uint32_t i = me; i < p2; i += THREADS) {
      key[i] = i < df ? ((unsigned long long)K.d_post_text[begin + i] << 32) | i : ~0ull;
      if (i < df)
        cntl[i] = K.d_post_count[begin + i];
    }
    __syncthreads ();
    for (uint32_t kk = 2; kk <= p2; kk <<= 1)
      for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
        for (uint32_t q = me; q < p2 / 2; q += THREADS) {
          const uint32_t a = ((q & ~(jj - 1)) << 1) | (q & (jj - 1)), b = a | jj; /* the q-th pair of this step */
          const unsigned long long x = key[a], y = key[b];
          if ((x > y) == ((a & kk) == 0)) {
            key[a] = y;
            key[b] = x;
          }
        }
        __syncthreads ();
      }
    for (uint32_t i = me; i < df; i += THREADS) {
      const unsigned long long w = key[i];
      K.d_post_text[begin + i] = (uint32_t)(w >> 32);
      K.d_post_count[begin + i] = cntl[(uint32_t)w];
    }
    __syncthreads (); /* (the next list sorts in the same words) */
  }
}

/* pass 6, behind the sort */
__global__ __launch_bounds__ (256) void
index_wide_put_kernel (IndexK K) {
  if (rules_stopped (K.G) || !index_fills (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < K.post_capacity; j += stride) {
    const unsigned long long w = K.skey[j];
    if (w == ~0ull) /* a sentinel: the room behind the wide entries */
      continue;
    const uint64_t k = w >> INDEX_TEXT_BITS;
    if (k >= K.n_keywords) {
      bad = true;
      continue;
    }
    const unsigned long long begin = K.ptr[k], df = K.ptr[k + 1] - begin, in_front = K.wbase[k];
    if (j < in_front || j - in_front >= df) { /* (a row that repeats a keyword, never tally_batch's: reported, left out) */
      bad = true;
      continue;
    }
    K.d_post_text[begin + (j - in_front)] = (uint32_t)(K.text_base + (w & ((1ull << INDEX_TEXT_BITS) - 1)));
    K.d_post_count[begin + (j - in_front)] = K.sval[j];
  }
  if (bad && K.G.error)
    *K.G.error = 1;
}

/* ------------------------------------------------------------------ CONCAT */
struct IndexCatK {
  const unsigned long long *a_ptr, *b_ptr, *a_count, *b_count;
  const uint32_t *a_text, *b_text;
  uint64_t n_a, n_b, out_capacity;
  RulesCtl *ctl; /* cleared in front of every call: bad = the inputs break the contract */
  unsigned long long *d_out_ptr, *d_out_nnz, *d_out_count;
  uint32_t *d_out_text;
  unsigned int *error;
};

/* out_ptr[k]: A's and B's entries in front of keyword k */
__device__ __forceinline__ unsigned long long
index_cat_ptr (const IndexCatK &C, uint64_t k) {
  return C.a_ptr[k < C.n_a ? k : C.n_a] + C.b_ptr[k];
}

/* BOUNDARY false: the pointer arrays begin with 0 and never decrease; true, in a launch of its own behind that one and
 * only when it found nothing: in every list B's first id lies above A's last */
template <bool BOUNDARY>
__global__ __launch_bounds__ (256) void
index_concat_check_kernel (IndexCatK C) {
  if (BOUNDARY && C.ctl->bad)
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = !BOUNDARY && blockIdx.x == 0 && threadIdx.x == 0 && (C.a_ptr[0] != 0 || C.b_ptr[0] != 0);
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < C.n_b; k += stride) {
    if (!BOUNDARY) {
      bad |= C.b_ptr[k] > C.b_ptr[k + 1];
      if (k < C.n_a)
        bad |= C.a_ptr[k] > C.a_ptr[k + 1];
    } else if (k < C.n_a) {
      const unsigned long long ab = C.a_ptr[k], ae = C.a_ptr[k + 1], bb = C.b_ptr[k], be = C.b_ptr[k + 1];
      if (ae > ab && be > bb)
        bad |= C.b_text[bb] <= C.a_text[ae - 1];
    }
  }
  if (bad) {
    C.ctl->bad = 1;
    if (C.error)
      *C.error = 1;
  }
}

__global__ __launch_bounds__ (256) void
index_concat_finish_kernel (IndexCatK C) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool stop = C.ctl->bad != 0;
  if (me == 0)
    *C.d_out_nnz = stop ? 0ull : index_cat_ptr (C, C.n_b);
  if (stop) /* every other output stays as it was */
    return;
  for (uint64_t k = me; k <= C.n_b; k += stride)
    C.d_out_ptr[k] = index_cat_ptr (C, k);
}

__global__ __launch_bounds__ (256) void
index_concat_fill_kernel (IndexCatK C) {
  if (C.ctl->bad)
    return;
  const unsigned long long n = index_cat_ptr (C, C.n_b);
  if (n > C.out_capacity)
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    /* the keyword of entry e: the last list that begins at or in front of e */
    uint64_t k = 0, hi = C.n_b;
    while (k < hi) {
      const uint64_t mid = k + ((hi - k) >> 1);
      if (index_cat_ptr (C, mid + 1) <= e)
        k = mid + 1;
      else
        hi = mid;
    }
    const unsigned long long off = e - index_cat_ptr (C, k), from_a = k < C.n_a ? C.a_ptr[k + 1] - C.a_ptr[k] : 0ull;
    if (off < from_a) {
      C.d_out_text[e] = C.a_text[C.a_ptr[k] + off];
      C.d_out_count[e] = C.a_count[C.a_ptr[k] + off];
    } else {
      C.d_out_text[e] = C.b_text[C.b_ptr[k] + off - from_a];
      C.d_out_count[e] = C.b_count[C.b_ptr[k] + off - from_a];
    }
  }
}
