/* dev_anchored.h -- anchored matches and dictionary lookup: ANCHORED and LOOKUP of a batch (include/acm_gpu.h).
 * Device code of libac75_amd.so; included by acm_gpu.hip inside its anonymous namespace.
 *
 * The keywords that are PREFIXES of text t are the terminal states on the one goto path that text t
 * spells from the root: no failure link is followed, no position but the text's first is a start, and
 * the path ends at the first missing edge or after min (|text t|, lmax) symbols.  So this family runs
 * no scan kernel and filters no record set: one lane takes one text and walks it, anchored_walk.
 * Which table a trie is walked in (AnchoredTrie; the kernels' STARTS argument): the start-parallel
 * tables of a plan that acm_gpu_plan_update edits in place (srec / sedge / the root table, and the
 * oinfo that goes with them -- the plan's CSR copy goes stale), the CSR goto rows of every other plan
 * and of every delta (csr_step's row search without its failure loop).  A plan with a delta walks both tries in lockstep on the same
 * position: two keywords never share a spelling, so at most one of the two states is terminal at any
 * depth and the records of a text come out by ascending length with no merge.  A state s reached
 * after d symbols is a keyword's end iff oinfo[s] has outputs and its first output's length is d
 * (the first output of a state is its longest: the state's own keyword when it is terminal).
 * Behind offsets_check_kernel (dev_batch.h; the batch contract on offsets[]: first 0, last n_symbols,
 * non-decreasing, checked in a launch of its own so that no address is formed from an offset the
 * check has not seen), two passes with a prefix sum between them (hipCUB, 64-bit, over n_texts + 1
 * entries):
 *   1. anchored_count_kernel: a lane walks its text and writes count[t], the records the mode keeps
 *      of it.  The lookup call ends here: the same walk writes whole_id / prefix_id / prefix_len.
 *   2. anchored_fill_kernel: walks the text again (the tables stay in L2 and the walk is short:
 *      nothing is kept between the passes) and stores record j of text t at first[t] + j as one
 *      16-byte store, text_id beside it; the lane of text t also writes d_first[t], the lane behind
 *      the last text d_first[n_texts] and *d_count.
 * Every output slot is written once, by one lane; no atomics.  A symbol is one naturally aligned load,
 * never of a symbol at or behind offsets[t + 1].  Launch geometry never depends on what the texts
 * hold: capped grids, grid-stride loops over the texts. */
constexpr uint32_t ANCHORED_THREADS = 256;
constexpr uint32_t ANCHORED_GRID_MAX = 1u << 20; /* ACM_GPU_ANCHORED_GRID's largest value */

/* control words at the head of the call's scratch, cleared in front of every call */
struct AnchoredCtl {
  unsigned int bad; /* offsets[] break the batch contract: nothing is walked */
  unsigned int pad[3];
};

/* one trie as the walk reads it, in one of two forms: the CSR goto rows (CsrTables: rows sorted by
 * symbol), or the start-parallel tables (StartsK) of a plan that acm_gpu_plan_update edits in place.
 * The kernels are instantiated per form of the plan's own trie; a delta is never edited in place and
 * is always walked in its CSR rows. */
struct AnchoredTrie {
  union { /* the three tables of the form the kernel is instantiated for */
    struct {
      const uint32_t *row_ptr, *edge_sym, *edge_next; /* CsrTables' */
    } csr;
    struct {
      const uint4 *srec;   /* 2 x uint4 per state */
      const uint2 *sedge;  /* per goto edge */
      const uint32_t *lut; /* the root table */
    } starts;              /* StartsK's */
  };
  uint32_t lut_size; /* start-parallel: symbols the root table holds */
  uint32_t live;     /* the trie has an edge (0: nothing to walk, e.g. no delta) */
  const uint4 *oinfo;
  const unsigned char *text; /* what the trie's plan walks: the caller's symbols, class ids, interned ids */
};

struct AnchoredK {
  AnchoredTrie base, delta;
  uint32_t lmax; /* the longest keyword of both */
  uint32_t mode; /* ACM_ANCHORED_*; 0: the lookup call */
  const unsigned long long *offsets; /* [n_texts + 1] */
  uint64_t n_texts, n_symbols;
  unsigned long long *count;       /* [n_texts + 1] records per text (the last entry stays 0) */
  const unsigned long long *first; /* [n_texts + 1] their exclusive prefix sum: [n_texts] = all records */
  ACMRecord *records;
  uint32_t *text_id;       /* may be NULL */
  unsigned long long *d_first; /* may be NULL */
  uint64_t capacity;
  unsigned long long *d_count;
  uint32_t *whole_id, *prefix_id, *prefix_len; /* lookup: each may be NULL */
  AnchoredCtl *ctl;
  unsigned int *error; /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* symbol i of a walked text: one naturally aligned load */
template <int SB>
__device__ __forceinline__ uint32_t
anchored_symbol (const unsigned char *text, uint64_t i) {
  const unsigned char *p = text + i * SB;
  if (SB == 1)
    return *p;
  if (SB == 2)
    return *reinterpret_cast<const unsigned short *> (p);
  return *reinterpret_cast<const unsigned int *> (p);
}

/* goto (s, c), NONE where the trie has no such edge */
template <bool STARTS>
__device__ __forceinline__ uint32_t
anchored_goto (const AnchoredTrie &T, uint32_t s, uint32_t c) {
  if (STARTS) { /* the tables acm_gpu_plan_update maintains: mirror_child's reading of them */
    const uint4 *srec = T.starts.srec;
    const uint2 *sedge = T.starts.sedge;
    if (s == 0 && c < T.lut_size) { /* the root table answers for the symbols it holds */
      const uint32_t e = T.starts.lut[c] & ST_STATE;
      return e ? e : NONE;
    }
    const uint4 ra = srec[2 * (size_t)s];
    const uint32_t ne = ra.y;
    if (ne <= 2 && s != 0) {
      const uint4 rb = srec[2 * (size_t)s + 1];
      if (ne >= 1 && rb.x == c)
        return rb.y;
      if (ne >= 2 && rb.z == c)
        return rb.w;
      return NONE;
    }
    uint32_t lo = ra.z, hi = ra.z + ne;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (sedge[mid].x < c)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < ra.z + ne) {
      const uint2 e = sedge[lo];
      if (e.x == c)
        return e.y;
    }
    return NONE;
  }
  uint32_t b = T.csr.row_ptr[s], e = T.csr.row_ptr[s + 1]; /* csr_step's row search */
  if (e - b > 8) {
    while (e - b > 1) {
      const uint32_t m = (b + e) >> 1;
      if (T.csr.edge_sym[m] <= c)
        b = m;
      else
        e = m;
    }
    return T.csr.edge_sym[b] == c ? T.csr.edge_next[b] : NONE;
  }
  for (; b < e; b++)
    if (T.csr.edge_sym[b] == c)
      return T.csr.edge_next[b];
  return NONE;
}

/* one step of one trie on symbol c at depth d (the symbols read so far): the state moves along the
 * goto edge or the trie is left for good; true when a keyword of length d ends here (kw: its id) */
template <bool STARTS>
__device__ __forceinline__ bool
anchored_step (const AnchoredTrie &T, bool &alive, uint32_t &s, uint32_t c, uint32_t d, uint32_t &kw) {
  s = anchored_goto<STARTS> (T, s, c);
  alive = s != NONE;
  if (!alive)
    return false;
  const uint4 oi = T.oinfo[s];
  kw = oi.w;
  return oi.x != 0 && oi.z == d;
}

/* the keywords that are prefixes of the text [begin, begin + len), by ascending length: found (length, keyword id) */
template <int SB, bool STARTS, typename F>
__device__ __forceinline__ void
anchored_walk (const AnchoredK &K, uint64_t begin, uint64_t len, F found) {
  const uint32_t steps = len < K.lmax ? (uint32_t)len : K.lmax;
  const bool one_text = K.delta.text == K.base.text; /* (uniform) */
  bool in_base = K.base.live != 0, in_delta = K.delta.live != 0;
  uint32_t sb = 0, sd = 0;
  for (uint32_t d = 1; d <= steps && (in_base || in_delta); d++) {
    const uint64_t i = begin + d - 1; /* below begin + len = offsets[t + 1] */
    const uint32_t c = anchored_symbol<SB> (K.base.text, i);
    uint32_t kw = 0;
    if (in_base && anchored_step<STARTS> (K.base, in_base, sb, c, d, kw))
      found (d, kw);
    if (in_delta && anchored_step<false> (K.delta, in_delta, sd, one_text ? c : anchored_symbol<SB> (K.delta.text, i), d, kw))
      found (d, kw);
  }
}

/* pass 1, and the whole of the lookup call */
template <int SB, bool STARTS>
__global__ __launch_bounds__ (ANCHORED_THREADS) void
anchored_count_kernel (AnchoredK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = K.ctl->bad != 0;
  for (uint64_t t = me; t <= K.n_texts; t += stride) {
    if (t == K.n_texts || bad) { /* the prefix sum still reads the entry */
      if (K.mode)
        K.count[t] = 0;
      continue;
    }
    const uint64_t begin = K.offsets[t], len = K.offsets[t + 1] - begin;
    uint32_t n = 0, longest = 0, longest_kw = NONE, whole_kw = NONE;
    bool whole = false;
    anchored_walk<SB, STARTS> (K, begin, len, [&] (uint32_t length, uint32_t kw) {
      n++;
      longest = length;
      longest_kw = kw;
      if (length == len) {
        whole = true;
        whole_kw = kw;
      }
    });
    if (K.mode)
      K.count[t] = K.mode == ACM_ANCHORED_PREFIXES ? n : K.mode == ACM_ANCHORED_LONGEST ? (n != 0) : whole;
    if (K.whole_id)
      K.whole_id[t] = whole_kw;
    if (K.prefix_id)
      K.prefix_id[t] = longest_kw;
    if (K.prefix_len)
      K.prefix_len[t] = longest;
  }
}

/* pass 2 */
template <int SB, bool STARTS>
__global__ __launch_bounds__ (ANCHORED_THREADS) void
anchored_fill_kernel (AnchoredK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = K.ctl->bad != 0;
  const unsigned long long total = K.first[K.n_texts];
  const bool room = total <= K.capacity; /* else: the count and d_first only, no record */
  for (uint64_t t = me; t <= K.n_texts; t += stride) {
    if (t == K.n_texts)
      *K.d_count = bad ? 0ull : total;
    if (bad)
      continue;
    const unsigned long long at = K.first[t];
    if (K.d_first)
      K.d_first[t] = at;
    if (t == K.n_texts || !room)
      continue;
    const unsigned long long end = K.first[t + 1];
    if (end == at)
      continue;
    const uint64_t begin = K.offsets[t], len = K.offsets[t + 1] - begin;
    uint32_t j = 0, keep_len = 0, keep_kw = 0;
    auto store = [&] (uint32_t length, uint32_t kw) {
      if (at + j >= end) /* (never expected: pass 1 walked the same text) */
        return;
      const uint64_t end_pos = begin + length - 1;
      *reinterpret_cast<uint4 *> (&K.records[at + j]) = make_uint4 ((uint32_t)end_pos, (uint32_t)(end_pos >> 32), length, kw);
      if (K.text_id)
        K.text_id[at + j] = (uint32_t)t;
      j++;
    };
    anchored_walk<SB, STARTS> (K, begin, len, [&] (uint32_t length, uint32_t kw) {
      if (K.mode == ACM_ANCHORED_PREFIXES)
        store (length, kw);
      else if (K.mode == ACM_ANCHORED_LONGEST || length == len) {
        keep_len = length;
        keep_kw = kw;
      }
    });
    if (K.mode != ACM_ANCHORED_PREFIXES && keep_len) /* (one record: pass 1 counted it) */
      store (keep_len, keep_kw);
  }
}
