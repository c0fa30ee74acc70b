/* dev_cooccur.h -- the keyword co-occurrence matrix of a batch: the upper triangle of C^T C (or of its
 * binary form) of the text x keyword count matrix C in CSR form, and the sum of two such matrices
 * (include/acm_cooccur.h).
 * Device code of libac75_amd.so; included by dev_all.h inside its anonymous namespace.
 *
 * The passes of the matrix, all on the caller's stream:
 *   1. rules_check_kernel (dev_rules.h): row_ptr[] begins with 0 and never decreases, or the call stops
 *      (the plan's error flag; no later pass forms an address from a row pointer then).
 *   2. cooccur_count_kernel: a lane per text; p[t] = r (r - 1) / 2 (+ r with DIAGONAL) for a row of r
 *      entries, 0 for a row above row_limit, which is counted in `skipped`.  An exclusive sum (hipCUB)
 *      gives pbase[]; cooccur_finish_kernel writes *d_cross and *d_skipped and stops the call when the
 *      cross room is too small (CoCtl::over).
 *   3. cooccur_expand_kernel: a lane per slot q of the cross room.  q < cross finds its text by bisection
 *      in pbase[] (neighbouring lanes share the path), its place (i, j) in the row's triangle from the
 *      triangular root -- taken in floating point, put right by integer compares, so exact for every q --
 *      and writes the key a << kb | b (kb: the bits that hold n_keywords itself, so that an all-ones a is no
 *      keyword) and, under PRODUCT, the weight C[t][a] * C[t][b].  A slot q >= cross, and a pair with a col
 *      that is no keyword, get the all-ones sentinel.
 *   4. A radix sort (hipCUB) of the room by the key's 2 kb live bits: keys alone without PRODUCT (the
 *      weights are all 1: half the traffic), pairs with it and in ADD.  The a-field of a sentinel is all
 *      ones within those bits too, which no keyword is: it sorts behind every real key and never equals
 *      one.  The sort runs over the whole room whatever it holds, so its launches depend on no count on
 *      the device.  cooccur_heads_kernel marks an entry that differs from its predecessor and is no
 *      sentinel; an exclusive sum of the marks gives every entry's rank, and the last is nnz.
 *   5. With weights, an inclusive sum of them modulo 2^64 into the sort's spare value buffer.
 *   6. cooccur_ptr_kernel: a lane per keyword a finds the lower bound of a << kb in the sorted keys and
 *      reads the rank there: co_ptr[a].  This needs no output room, so co_ptr is complete on an output
 *      overflow.
 *   7. The fill, only when nnz fits: cooccur_starts_kernel writes every run's first position to
 *      start[rank] (the sort's spare key buffer), and the end of the real entries to start[nnz];
 *      cooccur_fill_kernel, a lane per output entry e: col from the key at start[e], value = start[e + 1]
 *      - start[e] (the run's length), or the difference of the running sums at the run's two ends, which
 *      is exact under wrap.  No atomic decides a result, and a run as long as the batch costs what a
 *      short one does.
 * ADD feeds the entries of A and B (cooccur_add_feed_kernel: the key from the row found by bisection in
 * its pointer array, the value as the weight) into passes 4 to 7, behind a check of both pointer arrays
 * (cooccur_add_check_kernel).
 * Scratch: 16 bytes per text (p, pbase), 40 per slot of the cross room (two keys, two weights, a mark and a
 * rank) and the sort's own; nothing per keyword. */
constexpr uint32_t COOCCUR_PRODUCT = 1u, COOCCUR_DIAGONAL = 2u; /* (ACM_COOCCUR_*) */
constexpr unsigned long long COOCCUR_SENTINEL = ~0ull;
constexpr unsigned long long COOCCUR_ROW_MOST = 1ull << 32; /* a row's pair instances count as this at the most: beyond any room */

/* control words behind the RulesCtl at the head of the scratch, cleared in front of every call */
struct CoCtl {
  unsigned long long skipped; /* texts above row_limit */
  unsigned int over;          /* the cross room is too small: every later pass stops */
  unsigned int pad;
};

struct CoK {
  RulesK G; /* the gate: rules_stopped (G) stops every pass; row_ptr, n_texts, ctl, error and the tally in front */
  const uint32_t *col;
  const unsigned long long *val;
  uint64_t n_keywords, row_limit, cross_capacity, out_capacity;
  uint64_t room;    /* slots of the sort room: max (cross_capacity, 1) */
  uint32_t flags;   /* COOCCUR_*; ADD runs the later passes under PRODUCT */
  uint32_t kb;      /* bits of a key's b-field: 2^kb - 1 >= n_keywords */
  /* ADD */
  const unsigned long long *a_ptr, *b_ptr, *a_val, *b_val;
  const uint32_t *a_col, *b_col;
  uint64_t n_a;
  /* scratch */
  CoCtl *cctl;
  unsigned long long *p;           /* [n_texts + 1] pair instances per text, the last stays 0 */
  const unsigned long long *pbase; /* [n_texts + 1] their exclusive sum */
  unsigned long long *key, *w;     /* [room] as the expansion fills them */
  const unsigned long long *skey;  /* the keys, sorted */
  const unsigned long long *wsum;  /* the inclusive sum of the sorted weights */
  uint32_t *start;                 /* [room + 1] (the spare key buffer: 8 bytes a slot) every run's first position */
  uint32_t *mark;                  /* [room + 1] heads, the last stays 0 */
  const uint32_t *rank;            /* [room + 1] their exclusive sum: rank[room] = nnz */
  /* outputs */
  unsigned long long *d_co_ptr, *d_nnz, *d_cross, *d_skipped, *d_co_val;
  uint32_t *d_co_col;
};

__device__ __forceinline__ bool
cooccur_stopped (const CoK &K) {
  return rules_stopped (K.G) || K.cctl->over != 0;
}

/* the entries the fill passes may write: all of them, when they fit */
__device__ __forceinline__ bool
cooccur_fills (const CoK &K) {
  return K.d_co_col != nullptr && K.rank[K.room] <= K.out_capacity;
}

/* pass 2 */
__global__ __launch_bounds__ (256) void
cooccur_count_kernel (CoK K) {
  if (rules_stopped (K.G))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t skipped = 0; /* (a lane strides over fewer than 2^32 texts) */
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < K.G.n_texts; t += stride) {
    const unsigned long long r = K.G.row_ptr[t + 1] - K.G.row_ptr[t];
    unsigned long long p = 0;
    if (K.row_limit && r > K.row_limit)
      skipped++;
    else if (r >= COOCCUR_ROW_MOST) /* (the product below would not fit) */
      p = COOCCUR_ROW_MOST;
    else {
      p = (K.flags & COOCCUR_DIAGONAL) ? r * (r + 1) / 2 : r * (r ? r - 1 : 0) / 2;
      p = p < COOCCUR_ROW_MOST ? p : COOCCUR_ROW_MOST;
    }
    K.p[t] = p;
  }
  for (int d = WAVE / 2; d > 0; d >>= 1)
    skipped += __shfl_xor (skipped, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0 && skipped)
    atomicAdd (&K.cctl->skipped, (unsigned long long)skipped); /* (a count: the order of the additions decides nothing) */
}

/* behind the sum of pass 2: one lane */
__global__ __launch_bounds__ (WAVE) void
cooccur_finish_kernel (CoK K) {
  if (threadIdx.x != 0 || blockIdx.x != 0)
    return;
  if (rules_stopped (K.G)) { /* every other output stays as it was */
    *K.d_nnz = 0;
    *K.d_cross = 0;
    return;
  }
  const unsigned long long cross = K.pbase[K.G.n_texts];
  *K.d_cross = cross;
  *K.d_skipped = K.cctl->skipped;
  if (cross > K.cross_capacity) {
    K.cctl->over = 1;
    *K.d_nnz = 0;
  }
}

/* the place (i, j) of pair m in a row's triangle, pairs in order of j, then i: i < j, or i <= j with DIAGONAL.  The pairs in
 * front of column j number base (j) = j (j - 1) / 2 (+ j); j is the greatest with base (j) <= m.  (m < 2^32: a row's share) */
__device__ __forceinline__ void
cooccur_decode (unsigned long long m, bool diagonal, uint32_t &i, uint32_t &j) {
  const unsigned long long d = diagonal ? 1 : 0;
  /* base (j) <= m  <=>  j <= (sqrt (8 m + 1) + 1) / 2 - d; the float root is off by a few units at the most */
  long long g = (long long)((sqrtf ((float)(8 * m + 1)) + 1.0f) * 0.5f) - (long long)d;
  unsigned long long jj = g < (long long)(1 - d) ? 1 - d : (unsigned long long)g;
  while (jj > 1 - d && jj * (jj - 1) / 2 + d * jj > m)
    jj--;
  while ((jj + 1) * jj / 2 + d * (jj + 1) <= m)
    jj++;
  j = (uint32_t)jj;
  i = (uint32_t)(m - (jj * (jj - 1) / 2 + d * jj));
}

/* pass 3 */
__global__ __launch_bounds__ (256) void
cooccur_expand_kernel (CoK K) {
  if (cooccur_stopped (K))
    return;
  const unsigned long long cross = K.pbase[K.G.n_texts];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const bool product = (K.flags & COOCCUR_PRODUCT) != 0, diagonal = (K.flags & COOCCUR_DIAGONAL) != 0;
  bool bad = false;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < K.room; q += stride) {
    unsigned long long key = COOCCUR_SENTINEL, w = 0;
    if (q < cross) {
      /* the text of slot q: the last whose pairs begin at or in front of q (the texts without pairs in front of it begin there too) */
      uint64_t t = 0, hi = K.G.n_texts;
      while (t < hi) {
        const uint64_t mid = t + ((hi - t) >> 1);
        if (K.pbase[mid + 1] <= q)
          t = mid + 1;
        else
          hi = mid;
      }
      if (t < K.G.n_texts) { /* (q < cross = pbase[n_texts]: always) */
        const unsigned long long begin = K.G.row_ptr[t], r = K.G.row_ptr[t + 1] - begin;
        uint32_t i, j;
        cooccur_decode (q - K.pbase[t], diagonal, i, j);
        if (j < r) { /* (the pairs of a row of r entries: always) */
          uint32_t a = K.col[begin + i], b = K.col[begin + j];
          if (a > b) { /* (a row that does not ascend, never tally_batch's: the pair stays in the upper triangle) */
            const uint32_t s = a;
            a = b;
            b = s;
          }
          if (b >= K.n_keywords)
            bad = true;
          else {
            key = ((unsigned long long)a << K.kb) | b;
            if (product)
              w = K.val[begin + i] * K.val[begin + j];
          }
        }
      }
    }
    K.key[q] = key;
    if (product)
      K.w[q] = w;
  }
  if (bad && K.G.error)
    *K.G.error = 1;
}

/* pass 4, behind the sort */
__global__ __launch_bounds__ (256) void
cooccur_heads_kernel (CoK K) {
  if (cooccur_stopped (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= K.room; q += stride) {
    uint32_t head = 0;
    if (q < K.room) {
      const unsigned long long key = K.skey[q];
      head = key != COOCCUR_SENTINEL && (q == 0 || K.skey[q - 1] != key);
    }
    K.mark[q] = head;
  }
}

/* pass 6 */
__global__ __launch_bounds__ (256) void
cooccur_ptr_kernel (CoK K) {
  if (cooccur_stopped (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (me == 0)
    *K.d_nnz = K.rank[K.room];
  for (uint64_t a = me; a <= K.n_keywords; a += stride) {
    /* the first sorted key of row a or behind it; a = n_keywords: the first sentinel, or the room's end */
    const unsigned long long x = (unsigned long long)a << K.kb;
    uint64_t lo = 0, hi = K.room;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (K.skey[mid] < x)
        lo = mid + 1;
      else
        hi = mid;
    }
    K.d_co_ptr[a] = K.rank[lo];
  }
}

/* pass 7, first half */
__global__ __launch_bounds__ (256) void
cooccur_starts_kernel (CoK K) {
  if (cooccur_stopped (K) || !cooccur_fills (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < K.room; q += stride) {
    if (K.mark[q])
      K.start[K.rank[q]] = (uint32_t)q;
    /* the end of the real entries: the first sentinel, or the room's end */
    const bool real = K.skey[q] != COOCCUR_SENTINEL;
    if (!real && (q == 0 || K.skey[q - 1] != COOCCUR_SENTINEL))
      K.start[K.rank[K.room]] = (uint32_t)q;
    if (real && q + 1 == K.room)
      K.start[K.rank[K.room]] = (uint32_t)K.room;
  }
}

/* pass 7, second half */
__global__ __launch_bounds__ (256) void
cooccur_fill_kernel (CoK K) {
  if (cooccur_stopped (K) || !cooccur_fills (K))
    return;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n = K.rank[K.room];
  const bool weights = K.wsum != nullptr;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const uint32_t s = K.start[e], t = K.start[e + 1];
    if (s >= t || t > K.room) /* (runs are not empty and lie in the room: always) */
      continue;
    K.d_co_col[e] = (uint32_t)(K.skey[s] & ((1ull << K.kb) - 1));
    K.d_co_val[e] = weights ? K.wsum[t - 1] - (s ? K.wsum[s - 1] : 0ull) : (unsigned long long)(t - s);
  }
}

/* ------------------------------------------------------------------ ADD */
/* both pointer arrays begin with 0 and never decrease */
__global__ __launch_bounds__ (256) void
cooccur_add_check_kernel (CoK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = blockIdx.x == 0 && threadIdx.x == 0 && (K.a_ptr[0] != 0 || K.b_ptr[0] != 0);
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K.n_keywords; k += stride) {
    bad |= K.b_ptr[k] > K.b_ptr[k + 1];
    if (k < K.n_a)
      bad |= K.a_ptr[k] > K.a_ptr[k + 1];
  }
  if (bad) {
    K.G.ctl->bad = 1;
    if (K.G.error)
      *K.G.error = 1;
  }
}

/* one lane */
__global__ __launch_bounds__ (WAVE) void
cooccur_add_finish_kernel (CoK K) {
  if (threadIdx.x != 0 || blockIdx.x != 0)
    return;
  if (rules_stopped (K.G)) { /* every other output stays as it was */
    *K.d_nnz = 0;
    *K.d_cross = 0;
    return;
  }
  const unsigned long long na = K.a_ptr[K.n_a], nb = K.b_ptr[K.n_keywords];
  const unsigned long long cross = na + nb < na ? COOCCUR_SENTINEL : na + nb;
  *K.d_cross = cross;
  if (cross > K.cross_capacity) {
    K.cctl->over = 1;
    *K.d_nnz = 0;
  }
}

/* the row of entry e in ptr[0 .. n]: the last that begins at or in front of e */
__device__ __forceinline__ uint64_t
cooccur_row_of (const unsigned long long *ptr, uint64_t n, unsigned long long e) {
  uint64_t k = 0, hi = n;
  while (k < hi) {
    const uint64_t mid = k + ((hi - k) >> 1);
    if (ptr[mid + 1] <= e)
      k = mid + 1;
    else
      hi = mid;
  }
  return k;
}

/* ADD's pass 3: slot q is A's entry q, then B's entry q - nnz (A) */
__global__ __launch_bounds__ (256) void
cooccur_add_feed_kernel (CoK K) {
  if (cooccur_stopped (K))
    return;
  const unsigned long long na = K.a_ptr[K.n_a], all = na + K.b_ptr[K.n_keywords];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < K.room; q += stride) {
    unsigned long long key = COOCCUR_SENTINEL, w = 0;
    if (q < all) {
      const bool from_a = q < na;
      const unsigned long long e = from_a ? q : q - na;
      const uint64_t n = from_a ? K.n_a : K.n_keywords;
      const uint64_t a = cooccur_row_of (from_a ? K.a_ptr : K.b_ptr, n, e);
      const uint32_t b = from_a ? K.a_col[e] : K.b_col[e];
      if (a >= n || b >= K.n_keywords)
        bad = true;
      else {
        key = ((unsigned long long)a << K.kb) | b;
        w = from_a ? K.a_val[e] : K.b_val[e];
      }
    }
    K.key[q] = key;
    K.w[q] = w;
  }
  if (bad && K.G.error)
    *K.G.error = 1;
}
