/* dev_flows.h -- flow scans: batch texts that continue earlier ones (include/acm_gpu.h, ACMFlows).
 * Device code of libac75_amd.so; included by dev_all.h inside its anonymous namespace.
 *
 * The cursor after any symbol depends on the last lmax - 1 symbols only, so what a flow has to keep
 * between two calls is a SPELLING: its last min (lmax - 1, symbols seen) symbols, in the caller's
 * symbol size -- valid for every plan kind, for class and interned plans and for a plan with a
 * delta, where no single state id describes both automata.  A flow call places every text's carry
 * in front of the text in a second buffer, runs the batch scan (dev_batch.h) over that buffer and
 * keeps the records that end behind the carry.  The kernels around the scan, all grid-stride with
 * capped grids (the launch size depends on neither the number of texts nor of flows):
 *   1. flows_check_kernel: the contract on offsets[] and on the flow ids -- every id below n_flows,
 *      no flow twice in one call (one atomicExch of the call's sequence number per text on the
 *      flow's claim word).  A violation raises FlowsCtl::bad and the plan's error flag;
 *   2. flows_head_kernel: head[t] = the carry length of text t's flow (0 for an empty text, which
 *      takes no part, and for every text of a bad call); an exclusive sum (hipCUB) of it and
 *      flows_xoff_kernel give the expanded offsets xoff[t] = offsets[t] + the heads in front of t.
 *      The host does not know the sum, so the expanded buffer always has the worst-case length
 *      n_symbols + n_texts * (lmax - 1): what the heads leave free at its end is one more text,
 *      filled with zero symbols, none of whose records is kept;
 *   3. flows_gather_kernel: the one pass proportional to the text -- a group of lanes per text
 *      copies the flow's carry and then the text's symbols to their place, 16-byte stores on the
 *      destination's grid (the loads are aligned too where the phases agree), byte stores for the
 *      ends, which neighbouring texts share a 16-byte block with;
 *   4. the batch kernels with HEADS (dev_batch.h): a record is kept iff it lies inside its expanded
 *      text and ends at or behind xoff[t] + head[t]; its end_pos is rebased to the caller's buffer;
 *   5. flows_carry_kernel: the new carry of every non-empty text's flow, the last
 *      min (lmax - 1, head + length) symbols of its expanded text, read from the expanded buffer
 *      (no in-place hazard).  It reads the bad and overflow flags and writes nothing when one is
 *      set: a call that overflowed is simply repeated with room. */
constexpr uint32_t FLOWS_THREADS = 256;

struct FlowsCtl {
  unsigned int bad; /* offsets[] or the flow ids break the contract: no record, no carry changes */
  unsigned int pad[3];
};

struct FlowsK {
  const unsigned char *text; /* the caller's buffer */
  const uint64_t *offsets;   /* [n_texts + 1], the caller's */
  const uint32_t *flow;      /* [n_texts]; NULL: text t is flow t (n_texts <= n_flows is the host's check) */
  uint64_t n_texts, n_symbols, n_flows;
  uint32_t sb;         /* bytes per symbol of the caller's text */
  uint32_t keep;       /* lmax - 1: symbols of a full carry */
  uint32_t slot_bytes; /* of a flow's slot (a multiple of 16) */
  unsigned char *carry;
  uint32_t *carry_len, *claim;
  uint32_t seq;             /* this call's sequence number (never 0) */
  uint32_t *head;           /* [n_texts + 1] (the last entry is 0: the sum's total) */
  const uint64_t *head_sum; /* [n_texts + 1] exclusive sum of head */
  uint64_t *xoff;           /* [n_texts + 2] expanded offsets; the last text is the zero fill */
  unsigned char *expanded;
  uint64_t n_expanded;      /* n_symbols + n_texts * keep */
  uint32_t group_log2;      /* lanes per text: gather, carry-out */
  FlowsCtl *ctl;
  const BatchCtl *batch;    /* flows_carry_kernel: the scan's overflow and bad flags */
  unsigned int *error;      /* the plan's device-side flag (acm_gpu_plan_status) */
};

__global__ __launch_bounds__ (FLOWS_THREADS) void
flows_check_kernel (FlowsK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (me == 0)
    bad = K.offsets[0] != 0 || K.offsets[K.n_texts] != K.n_symbols;
  for (uint64_t t = me; t < K.n_texts; t += stride) {
    bad = bad || K.offsets[t] > K.offsets[t + 1];
    if (K.flow) {
      const uint32_t f = K.flow[t];
      if (f >= K.n_flows)
        bad = true;
      else if (atomicExch (&K.claim[f], K.seq) == K.seq) /* claimed in this call already */
        bad = true;
    }
  }
  if (bad) {
    K.ctl->bad = 1;
    if (K.error)
      *K.error = 1;
  }
}

__global__ __launch_bounds__ (FLOWS_THREADS) void
flows_head_kernel (FlowsK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = K.ctl->bad != 0;
  for (uint64_t t = me; t <= K.n_texts; t += stride) {
    uint32_t h = 0;
    if (!bad && t < K.n_texts && K.offsets[t + 1] > K.offsets[t]) {
      h = K.carry_len[K.flow ? K.flow[t] : t];
      if (h > K.keep) /* (lmax has shrunk since: never expected, a merge only adds keywords) */
        h = K.keep;
    }
    K.head[t] = h;
  }
}

/* a bad call scans zeros only: every real text empty, the fill all of the buffer */
__global__ __launch_bounds__ (FLOWS_THREADS) void
flows_xoff_kernel (FlowsK K) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = K.ctl->bad != 0;
  for (uint64_t t = me; t <= K.n_texts + 1; t += stride)
    K.xoff[t] = t > K.n_texts ? K.n_expanded : bad ? 0 : K.offsets[t] + K.head_sum[t];
}

/* n bytes from src to dst by the G lanes of a group (this is lane g): whole 16-byte blocks of the
 * destination's grid with one store each, the bytes in front of the first and behind the last
 * singly.  Nothing outside [dst, dst + n) is written. */
__device__ __forceinline__ void
flows_copy (unsigned char *__restrict__ dst, const unsigned char *__restrict__ src, uint64_t n, uint32_t g, uint32_t G) {
  uint64_t lead = (16 - (reinterpret_cast<uintptr_t> (dst) & 15)) & 15;
  if (lead > n)
    lead = n;
  for (uint64_t i = g; i < lead; i += G)
    dst[i] = src[i];
  const uint64_t blocks = (n - lead) / 16;
  if (((reinterpret_cast<uintptr_t> (dst) ^ reinterpret_cast<uintptr_t> (src)) & 15) == 0) {
    for (uint64_t b = g; b < blocks; b += G)
      *reinterpret_cast<uint4 *> (dst + lead + 16 * b) = *reinterpret_cast<const uint4 *> (src + lead + 16 * b);
  } else {
    for (uint64_t b = g; b < blocks; b += G) {
      uint4 v;
      __builtin_memcpy (&v, src + lead + 16 * b, 16); /* (a source off the grid) */
      *reinterpret_cast<uint4 *> (dst + lead + 16 * b) = v;
    }
  }
  for (uint64_t i = lead + 16 * blocks + g; i < n; i += G)
    dst[i] = src[i];
}

__global__ __launch_bounds__ (FLOWS_THREADS) void
flows_gather_kernel (FlowsK K) {
  const uint64_t threads = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = K.ctl->bad != 0;
  if (!bad) {
    const uint32_t G = 1u << K.group_log2, g = (uint32_t)me & (G - 1);
    const uint64_t groups = threads >> K.group_log2;
    for (uint64_t t = me >> K.group_log2; t < K.n_texts; t += groups) {
      const uint64_t begin = K.offsets[t], len = K.offsets[t + 1] - begin;
      if (len == 0)
        continue;
      const uint32_t h = K.head[t];
      unsigned char *dst = K.expanded + K.xoff[t] * K.sb;
      if (h)
        flows_copy (dst, K.carry + (uint64_t)(K.flow ? K.flow[t] : t) * K.slot_bytes, (uint64_t)h * K.sb, g, G);
      flows_copy (dst + (uint64_t)h * K.sb, K.text + begin * K.sb, len * K.sb, g, G);
    }
  }
  /* the zero fill behind the last text (all of the buffer in a bad call) */
  const uint64_t from = K.xoff[K.n_texts] * K.sb, to = K.n_expanded * K.sb;
  for (uint64_t b = from / 16 + me; b * 16 < to; b += threads) {
    const uint64_t at = b * 16;
    if (at >= from && at + 16 <= to)
      *reinterpret_cast<uint4 *> (K.expanded + at) = make_uint4 (0, 0, 0, 0);
    else
      for (uint64_t i = at < from ? from : at; i < at + 16 && i < to; i++)
        K.expanded[i] = 0;
  }
}

__global__ __launch_bounds__ (FLOWS_THREADS) void
flows_carry_kernel (FlowsK K) {
  if (K.ctl->bad || K.batch->bad || K.batch->overflow)
    return;
  const uint64_t threads = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t G = 1u << K.group_log2, g = (uint32_t)me & (G - 1);
  const uint64_t groups = threads >> K.group_log2;
  for (uint64_t t = me >> K.group_log2; t < K.n_texts; t += groups) {
    const uint64_t len = K.offsets[t + 1] - K.offsets[t];
    if (len == 0)
      continue;
    const uint64_t all = K.head[t] + len, keep = all < K.keep ? all : K.keep;
    const uint64_t f = K.flow ? K.flow[t] : t;
    /* (the end of text t's expanded symbols: xoff[t + 1] belongs to a later text only by name) */
    flows_copy (K.carry + f * K.slot_bytes, K.expanded + (K.xoff[t] + all - keep) * K.sb, keep * K.sb, g, G);
    if (g == 0)
      K.carry_len[f] = (uint32_t)keep;
  }
}

/* acm_gpu_flows_reset: flows back to the root (ids NULL: all of them) */
__global__ __launch_bounds__ (FLOWS_THREADS) void
flows_reset_kernel (uint32_t *carry_len, uint64_t n_flows, const uint32_t *ids, uint64_t n, unsigned int *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, me = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t i = me; i < (ids ? n : n_flows); i += stride) {
    const uint64_t f = ids ? ids[i] : i;
    if (f < n_flows)
      carry_len[f] = 0;
    else if (error)
      *error = 1;
  }
}
