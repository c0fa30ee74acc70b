/* dev_rules.h -- keyword rules per text: which rules of a set fire in which text of a batch, given
 * the text x keyword count matrix in CSR form (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The rule set lies on the device as an index inverted by keyword (acm_gpu_rules_create): the
 * postings (rule, lo, hi) of every keyword, base[r] = the terms of r that hold at count 0, need[r],
 * and the ascending list of the always-rules (base >= need).  A text's row then decides only about
 * the rules its keywords have postings for: every posting whose holding at the row's count differs
 * from its holding at count 0 is an ITEM (rule, +1 or -1), the items of a rule are added up, and
 * rule r fires iff base[r] + sum >= need[r].  A rule no item touched behaves as on an empty row: it
 * fires iff it is an always-rule.  The passes, all on the caller's stream:
 *   1. rules_check_kernel: row_ptr[] begins with 0 and never decreases, or the call stops (the
 *      plan's error flag; no later pass forms an address from a row pointer then).
 *   2. COUNT: rules_fast_kernel<false>, one wave (a block of 64 lanes: its barriers are the wave's
 *      own) per text, grid-stride.  A lane takes a row entry and walks its postings; items go into
 *      the wave's LDS at a slot from an LDS counter, as one word rule << 1 | (+1 ? 1 : 0).  A text
 *      with more items than the room (ACM_GPU_RULES_ITEMS, 1,024) goes on the list of WIDE texts.
 *      Otherwise: a bitonic sort of the words (padded with all ones to a power of two), the first
 *      word of every rule is its HEAD and adds up its run, the heads are compacted in place as
 *      rule << 1 | fires with d[h] = (firing heads in front) - (heads of always-rules in front).
 *      The row has (firing heads) + (always-rules) - (heads of always-rules) entries.
 *      rules_wide_kernel<false>, RULES_WIDE_BLOCKS blocks of 256 lanes, runs the same code on the
 *      wide texts with the words in global scratch: room for every posting of the set, which a row
 *      without repeated keywords cannot exceed (a row that does raises the error flag and stays
 *      empty).  Slow and always correct, so that no input is refused.
 *   3. An exclusive sum of the counts (hipCUB) in scratch; rules_finish_kernel copies it to
 *      d_fired_ptr and writes *d_n_fired.  Through scratch, so that a stopped call writes nothing.
 *   4. FILL (when there is a d_fired and the total fits): both kernels again, <true>.  A firing head
 *      h of rule r goes to lower_bound (always, r) + d[h] of its row, the always-rule always[j] that
 *      is no head to j + d[lower_bound (heads, always[j])]: the merge of two sorted lists by ranks,
 *      so rows come out strictly ascending.
 * LDS of the fast form: items_p2 words and items + 1 ranks, 8 KiB at 1,024 items; sixteen one-wave
 * blocks are launched per CU and fit its 160 KiB; the largest room, 4,096 items, is 32 KiB.
 * Work per text: the postings of its row's keywords, a sort of its items, the always-list times
 * the logarithm of its heads.  Nothing is sized by n_texts x n_rules; nothing reads a count back to
 * the host.  The number of texts either form took is added to the set's two counters by the count
 * pass (acm_gpu_rules_info). */
constexpr uint32_t RULES_ITEMS_DEFAULT = 1024, RULES_ITEMS_MAX = 4096;
constexpr uint32_t RULES_FAST_PER_CU = 16;
constexpr uint32_t RULES_WIDE_THREADS = 256, RULES_WIDE_BLOCKS = 8;
constexpr uint32_t RULES_NO_MAX = 0xFFFFFFFFu;
static_assert ((RULES_ITEMS_MAX & (RULES_ITEMS_MAX - 1)) == 0 && RULES_ITEMS_MAX * 8 + 4 + 64 <= 64 * 1024, "the widest fast form sorts in one block's LDS");
static_assert ((RULES_ITEMS_DEFAULT & (RULES_ITEMS_DEFAULT - 1)) == 0 && RULES_FAST_PER_CU * (RULES_ITEMS_DEFAULT * 8 + 4 + 64) <= 160 * 1024,
               "sixteen one-wave blocks of the fast form share one CU");

struct RulePost {
  uint32_t rule, lo, hi;
};

/* control words at the head of the passes' scratch, cleared in front of every call */
struct RulesCtl {
  unsigned int bad; /* row_ptr[] breaks the contract */
  unsigned int pad;
  unsigned long long n_wide; /* texts on the wide list */
};

struct RulesK {
  /* the count matrix */
  const unsigned long long *row_ptr; /* [n_texts + 1] */
  const uint32_t *col;
  const unsigned long long *val;
  uint64_t n_texts;
  /* the rule set */
  const uint32_t *post_ptr; /* [n_keywords + 1] */
  const RulePost *post;     /* [n_postings] */
  const uint32_t *base, *need, *always;
  uint32_t n_keywords, n_always, n_postings;
  unsigned long long *forms; /* [2] texts of the fast form, of the wide form */
  /* the rooms */
  uint32_t items, items_p2; /* the fast form's, and the power of two its LDS holds */
  uint32_t wide_p2;         /* a power of two >= n_postings */
  /* scratch */
  unsigned long long *cnt;       /* [n_texts + 1] entries per row, the last stays 0 */
  const unsigned long long *ptr; /* [n_texts + 1] their exclusive sum */
  uint32_t *wide;                /* [n_texts + 1] the wide texts */
  uint32_t *wkey;                /* [RULES_WIDE_BLOCKS][wide_p2] */
  int32_t *wd;                   /* [RULES_WIDE_BLOCKS][n_postings + 1] */
  RulesCtl *ctl;
  /* a tally_batch in front of this call (acm_gpu_rules_device), or nullptr */
  const TbCtl *tb;
  uint64_t tb_capacity, tb_pair_capacity;
  /* outputs */
  unsigned long long *d_fired_ptr, *d_n_fired;
  uint32_t *d_fired;
  uint64_t fired_capacity;
  unsigned int *error; /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* the tally in front reported nothing: its matrix is not there */
__device__ __forceinline__ bool
rules_no_matrix (const RulesK &K) {
  return K.tb && (K.tb->batch.bad != 0 || K.tb->need > K.tb_capacity || K.tb->partial > K.tb_pair_capacity);
}

__device__ __forceinline__ bool
rules_stopped (const RulesK &K) {
  return rules_no_matrix (K) || K.ctl->bad != 0;
}

/* pass 1 */
__global__ __launch_bounds__ (256) void
rules_check_kernel (RulesK K) {
  if (rules_no_matrix (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < K.n_texts; t += stride) {
    const unsigned long long a = K.row_ptr[t], b = K.row_ptr[t + 1];
    bad |= a > b || (t == 0 && a != 0);
  }
  if (bad) {
    K.ctl->bad = 1;
    if (K.error)
      *K.error = 1;
  }
}

/* entries of the ascending a[0 .. n) below x */
__device__ __forceinline__ uint32_t
rules_lower_bound (const uint32_t *a, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* the same over the rules of the heads key[0 .. n) (rule << 1 | fires) */
__device__ __forceinline__ uint32_t
rules_heads_below (const uint32_t *key, uint32_t n, uint32_t rule) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((key[mid] >> 1) < rule)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* Text t by a block of THREADS lanes, every one of which calls (the barriers see every lane): its
 * count into cnt[t], or with FILL its row into d_fired.  key[] has room for `room` items rounded up
 * to a power of two, d[] for room + 1; s_n and s_heads[3 * THREADS / WAVE] are the block's.
 * True, and nothing written, when the text has more items than `room`. */
template <uint32_t THREADS, bool FILL>
__device__ __forceinline__ bool
rules_text (const RulesK &K, uint64_t t, uint32_t *key, int32_t *d, uint32_t room, uint32_t *s_n, uint32_t *s_heads) {
  constexpr uint32_t WAVES = THREADS / WAVE;
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  if (threadIdx.x == 0)
    *s_n = 0;
  __syncthreads ();
  /* the items: a lane per row entry, its postings one after the other */
  const unsigned long long rb = K.row_ptr[t], re = K.row_ptr[t + 1];
  for (unsigned long long e = rb + threadIdx.x; e < re; e += THREADS) {
    const uint32_t k = K.col[e];
    if (k >= K.n_keywords) /* a keyword the plan took later: in no rule */
      continue;
    const unsigned long long v = K.val[e];
    const uint32_t pe = K.post_ptr[k + 1];
    for (uint32_t p = K.post_ptr[k]; p < pe; p++) {
      const RulePost q = K.post[p];
      const bool now = v >= q.lo && (q.hi == RULES_NO_MAX || v <= q.hi), empty = q.lo == 0;
      if (now != empty) {
        const uint32_t at = atomicAdd (s_n, 1u);
        if (at < room)
          key[at] = (q.rule << 1) | (now ? 1u : 0u);
      }
    }
  }
  __syncthreads ();
  const uint32_t n = *s_n;
  if (n > room) /* (uniform in the block, as every condition below around a barrier) */
    return true;
  const unsigned long long out = FILL ? K.ptr[t] : 0ull;
  if (n == 0) { /* no rule touched: the always-rules as they are */
    if (!FILL) {
      if (threadIdx.x == 0)
        K.cnt[t] = K.n_always;
    } else
      for (uint32_t j = threadIdx.x; j < K.n_always; j += THREADS)
        if (out + j < K.fired_capacity)
          K.d_fired[out + j] = K.always[j];
    return false;
  }
  /* sorted by rule, a rule's -1 items in front of its +1 items */
  uint32_t p2 = 1;
  while (p2 < n)
    p2 <<= 1;
  for (uint32_t i = n + threadIdx.x; i < p2; i += THREADS)
    key[i] = 0xFFFFFFFFu;
  __syncthreads ();
  for (uint32_t k = 2; k <= p2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < p2; i += THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint32_t a = key[i], b = key[l];
          if ((a > b) == ((i & k) == 0)) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
      __syncthreads ();
    }
  /* the heads, compacted in place: a head's place is never behind the head itself, and a chunk
   * reads all it needs -- the runs of its heads reach forward only -- before it writes.  (The word in
   * front of a chunk may have been replaced by its own head, which holds the same rule.) */
  uint32_t heads = 0, firing = 0, always_heads = 0;
  for (uint32_t c0 = 0; c0 < n; c0 += THREADS) {
    const uint32_t i = c0 + threadIdx.x;
    uint32_t r = 0;
    bool head = false, fires = false, always = false;
    if (i < n) {
      r = key[i] >> 1;
      head = i == 0 || (key[i - 1] >> 1) != r;
    }
    if (head) {
      long long sum = 0;
      for (uint32_t j = i; j < n && (key[j] >> 1) == r; j++)
        sum += (key[j] & 1u) ? 1 : -1;
      const uint32_t b = K.base[r], nd = K.need[r];
      fires = (long long)b + sum >= (long long)nd;
      always = b >= nd;
    }
    const unsigned long long mh = __ballot (head), mf = __ballot (fires), ma = __ballot (always);
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
      key[h] = (r << 1) | (fires ? 1u : 0u);
      d[h] = (int32_t)(firing + bf + rank_below (mf)) - (int32_t)(always_heads + ba + rank_below (ma));
    }
    heads += ah;
    firing += af;
    always_heads += aa;
    __syncthreads ();
  }
  if (!FILL) {
    if (threadIdx.x == 0)
      K.cnt[t] = (unsigned long long)firing + K.n_always - always_heads;
    return false;
  }
  if (threadIdx.x == 0)
    d[heads] = (int32_t)firing - (int32_t)always_heads;
  __syncthreads ();
  for (uint32_t h = threadIdx.x; h < heads; h += THREADS) {
    const uint32_t w = key[h];
    if (w & 1u) {
      const unsigned long long at = out + (unsigned long long)((long long)rules_lower_bound (K.always, K.n_always, w >> 1) + d[h]);
      if (at < K.fired_capacity)
        K.d_fired[at] = w >> 1;
    }
  }
  for (uint32_t j = threadIdx.x; j < K.n_always; j += THREADS) {
    const uint32_t a = K.always[j];
    const uint32_t h = rules_heads_below (key, heads, a);
    if (h < heads && (key[h] >> 1) == a) /* touched: its head has spoken */
      continue;
    const unsigned long long at = out + (unsigned long long)((long long)j + d[h]);
    if (at < K.fired_capacity)
      K.d_fired[at] = a;
  }
  return false;
}

/* passes 2 and 4, the fast form: a block is one wave */
template <bool FILL>
__global__ __launch_bounds__ (WAVE) void
rules_fast_kernel (RulesK K) {
  extern __shared__ uint32_t rules_lds[]; /* [items_p2] words, [items + 1] ranks */
  __shared__ uint32_t s_n, s_heads[3];
  if (rules_stopped (K) || (FILL && K.ptr[K.n_texts] > K.fired_capacity))
    return;
  uint32_t *key = rules_lds;
  int32_t *d = reinterpret_cast<int32_t *> (rules_lds + K.items_p2);
  unsigned long long fast = 0, wide = 0;
  for (uint64_t t = blockIdx.x; t < K.n_texts; t += gridDim.x) { /* (uniform in the block) */
    const bool over = rules_text<WAVE, FILL> (K, t, key, d, K.items, &s_n, s_heads);
    if (FILL)
      continue;
    if (over && threadIdx.x == 0)
      K.wide[atomicAdd (&K.ctl->n_wide, 1ull)] = (uint32_t)t;
    fast += over ? 0 : 1;
    wide += over ? 1 : 0;
  }
  if (!FILL && threadIdx.x == 0) {
    if (fast)
      atomicAdd (&K.forms[0], fast);
    if (wide)
      atomicAdd (&K.forms[1], wide);
  }
}

/* the wide form: the same with the words in the block's share of scratch */
template <bool FILL>
__global__ __launch_bounds__ (RULES_WIDE_THREADS) void
rules_wide_kernel (RulesK K) {
  __shared__ uint32_t s_n, s_heads[3 * RULES_WIDE_THREADS / WAVE];
  if (rules_stopped (K) || (FILL && K.ptr[K.n_texts] > K.fired_capacity))
    return;
  const uint64_t n_wide = K.ctl->n_wide;
  uint32_t *key = K.wkey + (size_t)blockIdx.x * K.wide_p2;
  int32_t *d = K.wd + (size_t)blockIdx.x * ((size_t)K.n_postings + 1);
  for (uint64_t w = blockIdx.x; w < n_wide; w += gridDim.x) { /* (uniform in the block) */
    const uint32_t t = K.wide[w];
    const bool over = rules_text<RULES_WIDE_THREADS, FILL> (K, t, key, d, K.n_postings, &s_n, s_heads);
    if (over && threadIdx.x == 0) { /* a row that repeats a keyword (never tally_batch's): reported, left empty */
      if (!FILL)
        K.cnt[t] = 0;
      if (K.error)
        *K.error = 1;
    }
    __syncthreads (); /* (the next text sorts in the same words) */
  }
}

/* pass 3 */
__global__ __launch_bounds__ (256) void
rules_finish_kernel (RulesK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool stop = rules_stopped (K);
  if (me == 0)
    *K.d_n_fired = stop ? 0ull : K.ptr[K.n_texts];
  if (stop) /* every other output stays as it was */
    return;
  for (uint64_t t = me; t <= K.n_texts; t += stride)
    K.d_fired_ptr[t] = K.ptr[t];
}
