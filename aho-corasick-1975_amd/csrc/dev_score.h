/* dev_score.h -- weighted keyword scores per text: the kept part of the text x class score matrix of a
 * count matrix in CSR form, the best class of every text, and the best k texts of every class
 * (include/acm_score.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace, behind
 * dev_rules.h, whose pass structure this is and whose row-pointer check (rules_check_kernel), stop
 * tests (rules_no_matrix, rules_stopped), finish kernel (rules_finish_kernel) and lower bound
 * (rules_lower_bound) run here as they are: a ScoreK begins with a RulesK that holds the matrix, the
 * index's post_ptr and always-list, the rooms, the scratch and the CSR outputs (d_fired_ptr is
 * d_kept_ptr, d_fired is d_kept_class, *d_n_fired is *d_n_kept).
 *
 * EVALUATION.  The model lies on the device as an index inverted by keyword (acm_gpu_score_create):
 * the postings (class, weight, cap) of every keyword, bias[], threshold[] and the ascending list of
 * the always-classes (bias >= threshold).  Every posting of every keyword of a row is an ITEM
 * (class, value = weight * min (count, cap) modulo 2^64).  The passes are dev_rules.h's:
 *   1. rules_check_kernel on d_row_ptr.
 *   2. COUNT: score_fast_kernel<false>, one wave (a block of 64 lanes) per text, grid-stride.  An
 *      item takes a slot from an LDS counter and is stored as a KEY class << 32 | slot and its value
 *      in val[slot].  Only the 8-byte keys go through the bitonic sort; a class's run then gathers
 *      its values once.  (Carrying the value through the sort would move 16 bytes per item and
 *      exchange instead of 8: the sort reads and writes every item log2 (n) * (log2 (n) + 1) / 2
 *      times, the gather once.)  The first key of a class is its HEAD and adds up its run; the heads
 *      are compacted in place as class << 32 | d, d = (kept heads in front) - (heads of
 *      always-classes in front).  The row has (kept heads) + (always-classes) - (heads of
 *      always-classes) entries.  A text with more items than the room (ACM_GPU_SCORE_ITEMS, 1,024)
 *      goes on the list of WIDE texts, which score_wide_kernel<false> takes with keys and values in
 *      global scratch: room for every posting of the model, which a row without repeated keywords
 *      cannot exceed (a row that does raises the error flag and stays empty).
 *   3. The exclusive sum of the counts; rules_finish_kernel writes d_kept_ptr and *d_n_kept.
 *   4. FILL (when there is room): both kernels again, <true>.  A kept head of class c writes its
 *      class and score at lower_bound (always, c) + d of its row while the heads are compacted; the
 *      always-class always[j] that is no head goes to j + d[lower_bound (heads, always[j])] with its
 *      bias as its score.  BEST is a reduction over (score, class) of everything the row writes.
 * LDS of the fast form: 8 bytes of key (rounded up to a power of two of items) and 8 bytes of value
 * per item, 16 KiB at 1,024 items; eight one-wave blocks are launched per CU (128 KiB of its 160; a
 * smaller room gets more by the same budget, sixteen at the most, a larger one fewer).
 * The largest room, 4,096 items, is 64 KiB of dynamic LDS beside the static words: the host raises
 * the kernel's limit for it.
 *
 * TOP.  Four passes over a kept matrix, none of whose launch geometry depends on a device count:
 *   1. score_top_hist_kernel: a lane per kept entry counts its class: class_hits.
 *   2. The exclusive sum of the counts: the column pointers.
 *   3. score_top_scatter_kernel: a lane per kept entry finds its text (an upper bound in kept_ptr)
 *      and puts the 128-bit key (score with its sign bit flipped, ~text) at a slot of its column taken
 *      from a cursor.  The order inside a column depends on the atomics; the result does not, because
 *      the order of the keys is total.
 *   4. score_top_select_kernel: a block of 256 lanes per class, grid-stride.  The running best 256 lie
 *      sorted in LDS; a tile of 256 candidates is read, those not above the current k-th are dropped,
 *      and if one is left the 512 keys are sorted again (bitonic, 8 KiB).  top_text and top_score are
 *      written once at the end.  One form for every k and every column length. */
constexpr uint32_t SCORE_ITEMS_DEFAULT = 1024, SCORE_ITEMS_MAX = 4096;
constexpr uint32_t SCORE_ITEM_BYTES = 16; /* key and value */
constexpr uint32_t SCORE_FAST_PER_CU = 8;
constexpr uint32_t SCORE_WIDE_THREADS = 256, SCORE_WIDE_BLOCKS = 8;
constexpr uint32_t SCORE_NO_CAP = 0xFFFFFFFFu, SCORE_NONE = 0xFFFFFFFFu;
constexpr uint32_t SCORE_TOP_THREADS = 256, SCORE_TOP_MAX = 256;
static_assert ((SCORE_ITEMS_MAX & (SCORE_ITEMS_MAX - 1)) == 0 && SCORE_ITEMS_MAX * SCORE_ITEM_BYTES + 64 <= 160 * 1024,
               "the widest fast form sorts in one block's LDS");
static_assert ((SCORE_ITEMS_DEFAULT & (SCORE_ITEMS_DEFAULT - 1)) == 0 && SCORE_FAST_PER_CU * (SCORE_ITEMS_DEFAULT * SCORE_ITEM_BYTES + 64) <= 160 * 1024,
               "eight one-wave blocks of the fast form share one CU");
static_assert (SCORE_TOP_MAX <= SCORE_TOP_THREADS && 2 * SCORE_TOP_THREADS * 16 <= 64 * 1024, "a lane per output of a class; 512 keys in LDS");

struct ScorePost {
  uint32_t cls;
  int32_t weight;
  uint32_t cap;
};

struct ScoreK {
  RulesK R; /* the part dev_rules.h's kernels and tests read (its post, base, need, wkey and wd stay unused) */
  const ScorePost *post; /* [n_postings] */
  const long long *bias, *threshold;
  unsigned long long *wkey; /* [SCORE_WIDE_BLOCKS][wide_p2] */
  unsigned long long *wval; /* [SCORE_WIDE_BLOCKS][n_postings] */
  long long *d_kept_score;
  uint32_t *d_best; /* or nullptr */
};

/* heads among the compacted key[0 .. n) (class << 32 | d) whose class is below cls */
__device__ __forceinline__ uint32_t
score_heads_below (const unsigned long long *key, uint32_t n, uint32_t cls) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((uint32_t)(key[mid] >> 32) < cls)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* a lane's candidate for BEST: the larger score, at a tie the smaller class; SCORE_NONE is no candidate */
__device__ __forceinline__ void
score_best_take (long long &bs, uint32_t &bc, long long s, uint32_t c) {
  if (c != SCORE_NONE && (bc == SCORE_NONE || s > bs || (s == bs && c < bc))) {
    bs = s;
    bc = c;
  }
}

/* best[t] of the block's candidates; every lane calls.  s_bs and s_bc have a word per wave. */
template <uint32_t THREADS>
__device__ __forceinline__ void
score_best_write (const ScoreK &K, uint64_t t, long long bs, uint32_t bc, long long *s_bs, uint32_t *s_bc) {
  constexpr uint32_t WAVES = THREADS / WAVE;
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const long long os = __shfl_xor (bs, off);
    const uint32_t oc = __shfl_xor (bc, off);
    score_best_take (bs, bc, os, oc);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    s_bs[threadIdx.x / WAVE] = bs;
    s_bc[threadIdx.x / WAVE] = bc;
  }
  __syncthreads ();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < WAVES; w++)
      score_best_take (bs, bc, s_bs[w], s_bc[w]);
    K.d_best[t] = bc;
  }
  __syncthreads (); /* (the next text's reduction writes the same words) */
}

/* Text t by a block of THREADS lanes, every one of which calls (the barriers see every lane): its
 * count into cnt[t], or with FILL its row into d_kept_class / d_kept_score and its best class.
 * key[] has room for `room` items rounded up to a power of two, val[] for `room`; s_n, s_tail,
 * s_heads[3 * THREADS / WAVE], s_bs and s_bc[THREADS / WAVE] are the block's.  True, and nothing
 * written, when the text has more items than `room`. */
template <uint32_t THREADS, bool FILL>
__device__ __forceinline__ bool
score_text (const ScoreK &K, uint64_t t, unsigned long long *key, unsigned long long *val, uint32_t room, uint32_t *s_n, int32_t *s_tail,
            uint32_t *s_heads, long long *s_bs, uint32_t *s_bc) {
  constexpr uint32_t WAVES = THREADS / WAVE;
  const RulesK &R = K.R;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  if (threadIdx.x == 0)
    *s_n = 0;
  __syncthreads ();
  /* the items: a lane per row entry, its postings one after the other */
  const unsigned long long rb = R.row_ptr[t], re = R.row_ptr[t + 1];
  for (unsigned long long e = rb + threadIdx.x; e < re; e += THREADS) {
    const uint32_t k = R.col[e];
    if (k >= R.n_keywords) /* a keyword the plan took later: in no term */
      continue;
    const unsigned long long v = R.val[e];
    const uint32_t pe = R.post_ptr[k + 1];
    for (uint32_t p = R.post_ptr[k]; p < pe; p++) {
      const ScorePost q = K.post[p];
      const unsigned long long capped = q.cap != SCORE_NO_CAP && v > q.cap ? q.cap : v;
      const uint32_t at = atomicAdd (s_n, 1u);
      if (at < room) {
        key[at] = ((unsigned long long)q.cls << 32) | at;
        val[at] = (unsigned long long)(long long)q.weight * capped;
      }
    }
  }
  __syncthreads ();
  const uint32_t n = *s_n;
  if (n > room) /* (uniform in the block, as every condition below around a barrier) */
    return true;
  const unsigned long long out = FILL ? R.ptr[t] : 0ull;
  long long bs = 0;
  uint32_t bc = SCORE_NONE;
  if (n == 0) { /* no class touched: the always-classes as they are */
    if (!FILL) {
      if (threadIdx.x == 0)
        R.cnt[t] = R.n_always;
      return false;
    }
    for (uint32_t j = threadIdx.x; j < R.n_always; j += THREADS) {
      const uint32_t a = R.always[j];
      const long long s = K.bias[a];
      if (out + j < R.fired_capacity) {
        R.d_fired[out + j] = a;
        K.d_kept_score[out + j] = s;
      }
      score_best_take (bs, bc, s, a);
    }
    if (K.d_best)
      score_best_write<THREADS> (K, t, bs, bc, s_bs, s_bc);
    return false;
  }
  /* sorted by class (the slots below keep the keys apart) */
  uint32_t p2 = 1;
  while (p2 < n)
    p2 <<= 1;
  for (uint32_t i = n + threadIdx.x; i < p2; i += THREADS)
    key[i] = ~0ull;
  __syncthreads ();
  for (uint32_t k = 2; k <= p2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < p2; i += THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const unsigned long long a = key[i], b = key[l];
          if ((a > b) == ((i & k) == 0)) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
      __syncthreads ();
    }
  /* the heads, compacted in place: a head's place is never behind the head itself, and a chunk
   * reads all it needs -- the runs of its heads reach forward only -- before it writes.  (The key in
   * front of a chunk may have been replaced by its own head, which holds the same class above.) */
  uint32_t heads = 0, kept = 0, always_heads = 0;
  for (uint32_t c0 = 0; c0 < n; c0 += THREADS) {
    const uint32_t i = c0 + threadIdx.x;
    uint32_t c = 0;
    bool head = false, keeps = false, always = false;
    long long score = 0;
    if (i < n) {
      c = (uint32_t)(key[i] >> 32);
      head = i == 0 || (uint32_t)(key[i - 1] >> 32) != c;
    }
    if (head) {
      const long long b = K.bias[c], th = K.threshold[c];
      unsigned long long sum = (unsigned long long)b;
      for (uint32_t j = i; j < n && (uint32_t)(key[j] >> 32) == c; j++)
        sum += val[(uint32_t)key[j]];
      score = (long long)sum;
      keeps = score >= th;
      always = b >= th;
    }
    const unsigned long long mh = __ballot (head), mf = __ballot (keeps), ma = __ballot (always);
    if (lane == 0) {
      s_heads[wave] = (uint32_t)__popcll (mh);
      s_heads[WAVES + wave] = (uint32_t)__popcll (mf);
      s_heads[2 * WAVES + wave] = (uint32_t)__popcll (ma);
    }
    __syncthreads ();
    uint32_t bh = 0, bf = 0, ba = 0, ah = 0, af = 0, aa = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) {
      bh += w < wave ? s_heads[w] : 0u;
      bf += w < wave ? s_heads[WAVES + w] : 0u;
      ba += w < wave ? s_heads[2 * WAVES + w] : 0u;
      ah += s_heads[w];
      af += s_heads[WAVES + w];
      aa += s_heads[2 * WAVES + w];
    }
    if (head) {
      const uint32_t h = heads + bh + rank_below (mh);
      const int32_t d = (int32_t)(kept + bf + rank_below (mf)) - (int32_t)(always_heads + ba + rank_below (ma));
      key[h] = ((unsigned long long)c << 32) | (uint32_t)d;
      if (FILL && keeps) {
        const unsigned long long at = out + (unsigned long long)((long long)rules_lower_bound (R.always, R.n_always, c) + d);
        if (at < R.fired_capacity) {
          R.d_fired[at] = c;
          K.d_kept_score[at] = score;
        }
        score_best_take (bs, bc, score, c);
      }
    }
    heads += ah;
    kept += af;
    always_heads += aa;
    __syncthreads ();
  }
  if (!FILL) {
    if (threadIdx.x == 0)
      R.cnt[t] = (unsigned long long)kept + R.n_always - always_heads;
    return false;
  }
  if (threadIdx.x == 0)
    *s_tail = (int32_t)kept - (int32_t)always_heads;
  __syncthreads ();
  for (uint32_t j = threadIdx.x; j < R.n_always; j += THREADS) {
    const uint32_t a = R.always[j];
    const uint32_t h = score_heads_below (key, heads, a);
    if (h < heads && (uint32_t)(key[h] >> 32) == a) /* touched: its head has spoken */
      continue;
    const int32_t d = h < heads ? (int32_t)(uint32_t)key[h] : *s_tail;
    const unsigned long long at = out + (unsigned long long)((long long)j + d);
    const long long s = K.bias[a];
    if (at < R.fired_capacity) {
      R.d_fired[at] = a;
      K.d_kept_score[at] = s;
    }
    score_best_take (bs, bc, s, a);
  }
  if (K.d_best)
    score_best_write<THREADS> (K, t, bs, bc, s_bs, s_bc);
  return false;
}

/* passes 2 and 4, the fast form: a block is one wave */
template <bool FILL>
__global__ __launch_bounds__ (WAVE) void
score_fast_kernel (ScoreK K) {
  extern __shared__ unsigned long long score_lds[]; /* [items_p2] keys, [items] values */
  __shared__ uint32_t s_n, s_heads[3], s_bc[1];
  __shared__ int32_t s_tail;
  __shared__ long long s_bs[1];
  const RulesK &R = K.R;
  if (rules_stopped (R) || (FILL && R.ptr[R.n_texts] > R.fired_capacity))
    return;
  unsigned long long *key = score_lds, *val = score_lds + R.items_p2;
  unsigned long long fast = 0, wide = 0;
  for (uint64_t t = blockIdx.x; t < R.n_texts; t += gridDim.x) { /* (uniform in the block) */
    const bool over = score_text<WAVE, FILL> (K, t, key, val, R.items, &s_n, &s_tail, s_heads, s_bs, s_bc);
    if (FILL)
      continue;
    if (over && threadIdx.x == 0)
      R.wide[atomicAdd (&R.ctl->n_wide, 1ull)] = (uint32_t)t;
    fast += over ? 0 : 1;
    wide += over ? 1 : 0;
  }
  if (!FILL && threadIdx.x == 0) {
    if (fast)
      atomicAdd (&R.forms[0], fast);
    if (wide)
      atomicAdd (&R.forms[1], wide);
  }
}

/* the wide form: the same with keys and values in the block's share of scratch */
template <bool FILL>
__global__ __launch_bounds__ (SCORE_WIDE_THREADS) void
score_wide_kernel (ScoreK K) {
  constexpr uint32_t WAVES = SCORE_WIDE_THREADS / WAVE;
  __shared__ uint32_t s_n, s_heads[3 * WAVES], s_bc[WAVES];
  __shared__ int32_t s_tail;
  __shared__ long long s_bs[WAVES];
  const RulesK &R = K.R;
  if (rules_stopped (R) || (FILL && R.ptr[R.n_texts] > R.fired_capacity))
    return;
  const uint64_t n_wide = R.ctl->n_wide;
  unsigned long long *key = K.wkey + (size_t)blockIdx.x * R.wide_p2;
  unsigned long long *val = K.wval + (size_t)blockIdx.x * R.n_postings;
  for (uint64_t w = blockIdx.x; w < n_wide; w += gridDim.x) { /* (uniform in the block) */
    const uint32_t t = R.wide[w];
    const bool over = score_text<SCORE_WIDE_THREADS, FILL> (K, t, key, val, R.n_postings, &s_n, &s_tail, s_heads, s_bs, s_bc);
    if (over && threadIdx.x == 0) { /* a row that repeats a keyword (never tally_batch's): reported, left empty */
      if (!FILL)
        R.cnt[t] = 0;
      if (R.error)
        *R.error = 1;
    }
    __syncthreads (); /* (the next text sorts in the same words) */
  }
}

/* ------------------------------------------------------------------ TOP */
struct ScoreTopK {
  RulesK G; /* the gate: rules_stopped (G) stops every pass.  A call of its own: row_ptr = the kept_ptr that rules_check_kernel
             * looks at first; behind an evaluation: the evaluation's own RulesK */
  const unsigned long long *kept_ptr; /* [n_texts + 1] */
  const uint32_t *kept_class;
  const long long *kept_score;
  uint64_t n_texts, kept_capacity;
  uint32_t n_classes, k;
  /* scratch */
  unsigned long long *hist;          /* [n_classes + 1] kept entries per class, the last stays 0; cleared in front of every call */
  unsigned long long *cursor;        /* [n_classes] slots taken in a column; cleared with hist */
  const unsigned long long *col_ptr; /* [n_classes + 1] the exclusive sum of hist */
  ulonglong2 *keys;                  /* [kept_capacity] x = ~text, y = the score with its sign bit flipped */
  /* outputs */
  unsigned long long *d_class_hits;
  uint32_t *d_top_n, *d_top_text;
  long long *d_top_score;
  unsigned int *error;
};

/* kept entries the passes read: none when the kept matrix had no room */
__device__ __forceinline__ unsigned long long
score_top_entries (const ScoreTopK &T) {
  const unsigned long long n = T.kept_ptr[T.n_texts];
  return n > T.kept_capacity ? 0ull : n;
}

/* pass 1 */
__global__ __launch_bounds__ (256) void
score_top_hist_kernel (ScoreTopK T) {
  if (rules_stopped (T.G))
    return;
  const unsigned long long n = score_top_entries (T);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const uint32_t c = T.kept_class[e];
    if (c < T.n_classes)
      atomicAdd (&T.hist[c], 1ull);
    else
      bad = true;
  }
  if (bad && T.error)
    *T.error = 1;
}

/* pass 3 */
__global__ __launch_bounds__ (256) void
score_top_scatter_kernel (ScoreTopK T) {
  if (rules_stopped (T.G))
    return;
  const unsigned long long n = score_top_entries (T);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const uint32_t c = T.kept_class[e];
    if (c >= T.n_classes)
      continue;
    /* the text of entry e: the last row that begins at or in front of e (the empty rows in front of it begin there too) */
    uint64_t lo = 0, hi = T.n_texts;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (T.kept_ptr[mid + 1] <= e)
        lo = mid + 1;
      else
        hi = mid;
    }
    const unsigned long long at = T.col_ptr[c] + atomicAdd (&T.cursor[c], 1ull);
    if (at < T.kept_capacity) /* (the columns' sizes add up to n: always) */
      T.keys[at] = make_ulonglong2 ((unsigned long long)(uint32_t)~(uint32_t)lo, (unsigned long long)T.kept_score[e] ^ (1ull << 63));
  }
}

__device__ __forceinline__ bool
score_key_above (unsigned long long ax, unsigned long long ay, unsigned long long bx, unsigned long long by) {
  return ay > by || (ay == by && ax > bx);
}

/* pass 4.  The empty key (0, 0) lies below every real one: a real x is ~text >= 2^31. */
__global__ __launch_bounds__ (SCORE_TOP_THREADS) void
score_top_select_kernel (ScoreTopK T) {
  __shared__ unsigned long long s_x[2 * SCORE_TOP_THREADS], s_y[2 * SCORE_TOP_THREADS];
  if (rules_stopped (T.G))
    return;
  const bool none = T.kept_ptr[T.n_texts] > T.kept_capacity;
  const uint32_t me = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < T.n_classes; c += gridDim.x) { /* (uniform in the block) */
    const unsigned long long hits = none ? 0ull : T.hist[c], begin = none ? 0ull : T.col_ptr[c];
    s_x[me] = 0;
    s_y[me] = 0;
    __syncthreads ();
    for (unsigned long long base = 0; T.k && base < hits; base += SCORE_TOP_THREADS) {
      unsigned long long x = 0, y = 0;
      if (base + me < hits && begin + base + me < T.kept_capacity) {
        const ulonglong2 q = T.keys[begin + base + me];
        x = q.x;
        y = q.y;
      }
      /* what cannot beat the current k-th is dropped (an empty k-th is beaten by every real key) */
      const bool stays = score_key_above (x, y, s_x[T.k - 1], s_y[T.k - 1]);
      s_x[SCORE_TOP_THREADS + me] = stays ? x : 0ull;
      s_y[SCORE_TOP_THREADS + me] = stays ? y : 0ull;
      if (__syncthreads_or (stays)) {
        /* the 512 keys in descending order: the best 256 in front */
        for (uint32_t kk = 2; kk <= 2 * SCORE_TOP_THREADS; kk <<= 1)
          for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            const uint32_t i = ((me & ~(j - 1)) << 1) | (me & (j - 1)), l = i | j; /* the me-th pair of this step */
            const unsigned long long ax = s_x[i], ay = s_y[i], bx = s_x[l], by = s_y[l];
            if (score_key_above (bx, by, ax, ay) == ((i & kk) == 0)) {
              s_x[i] = bx;
              s_y[i] = by;
              s_x[l] = ax;
              s_y[l] = ay;
            }
            __syncthreads ();
          }
      }
    }
    const unsigned long long top = hits < T.k ? hits : T.k;
    if (me == 0) {
      T.d_class_hits[c] = hits;
      T.d_top_n[c] = (uint32_t)top;
    }
    if (me < T.k) {
      const size_t at = (size_t)c * T.k + me;
      T.d_top_text[at] = me < top ? ~(uint32_t)s_x[me] : SCORE_NONE;
      T.d_top_score[at] = me < top ? (long long)(s_y[me] ^ (1ull << 63)) : 0ll;
    }
    __syncthreads (); /* (the next class clears the same words) */
  }
}
