/* dev_all.h -- the device side of libac75_amd.so as ONE unit: the constants and structs the kernels
 * share and the dev_*.h files that hold them, in an anonymous namespace.  acm_gpu.hip includes this
 * and adds the host side; tools/kernel_regs_one.sh compiles it alone with a single kernel
 * instantiated (seconds instead of the minutes the whole library takes). */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "acm_internal.h"

#ifdef ACM_GRAM_NT_BOTH /* experiment builds (make expd D=...): non-temporal text loads and record stores in the 4-gram kernel */
#define ACM_GRAM_NT_TEXT
#define ACM_GRAM_NT_REC
#endif

/* Diagnostic build only (-DACM_DIAG, libac75_amd_diag.so, used by tools/diag_*.py): eight per-wave
 * counters (cycle stamps, call counts) whose meaning each kernel defines where it writes them.
 * Nothing of this exists in the product build. */
#ifdef ACM_DIAG
__device__ unsigned long long g_acm_diag[8192][8];
#define DIAG(...) __VA_ARGS__
#else
#define DIAG(...)
#endif

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int WAVE = 64;
constexpr int QCAP = 128;           /* per-wave queue of (position, state) items, 8 B each */
constexpr uint32_t GRAM_Q2 = 96;    /* 4-gram kernel: per-wave queue of walk candidates */
/* 4-gram kernel: its first queue (63 items waiting + up to 64 from one position).  Two other forms
 * of the push -- the fill in a vector register with the exec mask narrowed around the LDS write
 * (9.6 % slower), four positions' compares ahead of their scalar counts (19 % slower: 217 scalar
 * and 115 vector registers spilled) -- are tools/experiments/r03_gram_push_variants.patch */
constexpr uint32_t GRAM_Q1 = 128;
constexpr uint32_t GRAM_NO_PEEK = 0xFFFFFFFFu; /* 4-gram kernel, GramK::g5peek: the state's record has to be looked at */
constexpr int DENSE_THREADS = 1024; /* one workgroup per CU, 16 waves */
/* dense kernel geometry: C = 64 bytes per lane-stream per tile, S = 2 streams per lane
 * (-DACM_DENSE_S=n builds another stream count for experiments: 3 and 4 spill and are 2x slower) */
#ifndef ACM_DENSE_S
#define ACM_DENSE_S 2
#endif
constexpr int DENSE_C = 64; /* (the kernel's template argument C; the slow step takes the stream stride 64 * C from here) */
/* a region must hold the items of two 16-step blocks beside a queue's worth: region_make_room */
constexpr uint32_t DENSE_MIN_REGION_ITEMS = 2 * (16 * ACM_DENSE_S * WAVE + QCAP);
/* continuation mode: straight-line run-over steps past a chunk before the lanes still inside a
 * match park a walk item (IT_WALK) and stop; -DACM_DENSE_RUNOVER=n builds another count */
#ifndef ACM_DENSE_RUNOVER
#define ACM_DENSE_RUNOVER 4
#endif
constexpr uint32_t DENSE_RUNOVER = ACM_DENSE_RUNOVER;
static_assert (DENSE_RUNOVER >= 1 && DENSE_RUNOVER <= 16, "the run-over steps read one 16-byte block past the chunk");
/* dense kernel: items go through a 128-item LDS queue per wave to the wave's HBM region.
 * -DACM_DENSE_DIRECT_PARK (experiment, slower: DESIGN.md 4.1) stores them straight from the slow
 * side into the region and gives the queues' 16 KiB to rows */
#ifdef ACM_DENSE_DIRECT_PARK
constexpr bool DENSE_LDS_QUEUE = false;
#else
constexpr bool DENSE_LDS_QUEUE = true;
#endif
constexpr uint64_t SEGMENT = 1ull << 31; /* symbols per launch: positions inside a launch are 32-bit */
/* tests shrink it with ACM_GPU_SEGMENT_LOG2 to cross segment seams on small inputs */

/* tables of the CSR kernel, states in breadth-first numbering (ACMFlatView) */
struct CsrTables {
  const uint32_t *row_ptr, *edge_sym, *edge_next, *fail, *nb_outputs;
  uint32_t lmax;
};

/* what turns a queued (position, state) into records; states in breadth-first numbering.
 * oinfo[s] = { nb_outputs(s), next, length, keyword_id } describes the FIRST output of s (the
 * longest keyword ending there: s itself if terminal, else the nearest terminal state down its
 * failure chain) and `next` = the terminal state holding the following one: one 16-byte load per
 * record.  The second half serves the continuations of the dense kernel. */
struct EmitCtx {
  const uint4 *oinfo;
  ACMRecord *records;
  unsigned long long *count; /* running total of records: slots are reserved by atomicAdd on it */
  uint64_t capacity, pos_base;
  const unsigned char *text;  /* segment */
  const uint32_t *wrows;      /* continuation rows of every state: next | out flag << 15 | depth(next) << 16 */
  const uint16_t *cont_dh;    /* per state: depth of the nearest failure-chain state whose row is in LDS */
  uint32_t W, lo, span, n, emit_from;
  uint32_t chunk; /* bytes per lane-stream chunk of the dense kernel (a power of two) */
  uint32_t n_states;
  unsigned int *error; /* set to 1 if an item with an impossible state id is ever met (never expected) */
  /* 4-gram kernels: keyword id of every depth-4 state by its rank among them (NONE: not a keyword).
   * A hit whose state word carries HIT_LEN4 names such a state by that rank: its record is
   * (position, 4, kw4[rank]) -- a 360 KB table that stays in L2 instead of the 16-byte output
   * records of all 508,339 states (config 3: 26 of 27 M hits per GiB are keywords of 4 symbols) */
  const uint32_t *kw4;
  /* dense kernel, continuation mode: per rowless state s (index s - chain_base) what lies below
   * it when that is ONE path to a leaf: { r | depth (hotfail (s)) << 4, leaf state t, the r <= 8
   * symbols of the path }; r = 0: no such record (walk_continuation goes step by step), r = 15:
   * s is a leaf.  NULL: none. */
  const uint4 *chain;
  uint32_t chain_base;
  /* 4-gram kernel, narrow alphabets: records are written by the scan kernel itself into chunks of
   * the caller's buffer (dev_starts.h: WaveRec); slots past `capacity` go to the plan's spill
   * area, from which close_holes_kernel brings them back into the holes below the dense count */
  uint4 *spill;
  uint64_t spill_slots;
  /* tiled scans (dev_tiles.h): `records` is a raw area of whole chunks, and a wave that reserves
   * chunk c writes chunk_prev[c] = the chunk it filled before (NONE: its first) */
  uint32_t *chunk_prev;
  /* slots per chunk of records a wave reserves with one atomic on the record counter: REC_CHUNK in
   * tiled scans (their directory counts in chunks of that size), REC_CHUNK_BIG in other scans of
   * long texts -- every wave of the chip adds to the same counter, 4.8 ns a time: a dictionary of
   * short keywords (164 M records from 2 GiB) spent 0.78 of 1.98 ms on 161 K reservations */
  uint32_t rec_chunk;
};
constexpr uint32_t HIT_LEN4 = 0x80000000u;
/* the hit's word is the keyword itself: id (below 2^28) | length << 28 (1-3; 0: 4 symbols) | HIT_KW -- what
 * the 4-gram kernel's tables hold for the keywords of up to 4 symbols, so that their records need
 * no lookup (one in 13 positions of a text can end such a keyword) */
constexpr uint32_t HIT_KW = 0x40000000u, HIT_KW_ID = 0x0FFFFFFFu;

/* one launch: a segment of the buffer, positions relative to its first symbol */
struct Launch {
  const unsigned char *text; /* first symbol of the segment */
  uint32_t n;                /* symbols in the segment */
  uint32_t emit_from;        /* matches ending before this index are not reported */
  uint32_t range_begin, range_end; /* dense: tile indices; csr: symbol indices */
  /* dense: tiles [range_begin, static_end) are split evenly between the blocks; [static_end,
   * range_end) is a pool in POOL_CLASSES equal parts, handed out tile by tile through pool_ctr */
  uint32_t static_end, pool_class_tiles;
  uint32_t pool_classes; /* min (POOL_CLASSES, blocks): block b draws from part b * pool_classes / blocks */
  unsigned int *pool_ctr, *pool_reset; /* this launch's counters; the previous launch's, to zero */
};
static constexpr uint32_t POOL_CLASSES = 16, POOL_CTR_STRIDE = 64; /* counters 256 B apart */

/* Dense kernel, continuation mode: hotfail (s) of the rowless states s = HD, HD + 1, ... lies in
 * LDS in DESCENDING order of address and ends at this compile-time address: hotfail (s) is the
 * 2 bytes at DENSE_HF_END - 2 - 2 * (s - HD), which the slow step forms from HD (in a scalar
 * register anyway: the fast side compares with it) and a literal, with no other kernel argument.
 * The rows, the queues and the tile counter lie below, from address 0; the gap between the two
 * parts is what the budget of build_dense leaves unused.  (The kernel runs on gfx950 only: 160 KiB
 * per workgroup; 512 bytes less 48 of rounding stay free as before.) */
constexpr uint32_t DENSE_LDS_CAP = 160 * 1024;
constexpr uint32_t DENSE_HF_END = DENSE_LDS_CAP - 512 + 48;
static_assert (DENSE_HF_END % 16 == 0 && DENSE_HF_END <= DENSE_LDS_CAP, "the hotfail part is staged in 16-byte pieces");

/* small uniform constants of the dense kernel */
struct DenseK {
  uint32_t W, rowbytes, lo, span;
  uint32_t HD; /* states [0, HD): failure-resolved row in LDS */
  uint32_t rows_bytes; /* the rows' part of the LDS image (a multiple of 16); the rest goes below DENSE_HF_END */
  uint32_t queue_off, wub, lmax;
  uint32_t stream_stride; /* 64 * C: distance between the chunks of a lane's consecutive streams */
};

/* queue item, second word, when the dense kernel runs in continuation mode (16-bit states) */
constexpr uint32_t IT_STATE = 0x7FFFu;
constexpr uint32_t IT_CONT = 1u << 15;  /* walk on from this (rowless) state: see walk_continuation */
constexpr uint32_t IT_K_SHIFT = 16;     /* 12 bits: run-over step k (symbols past the end of the lane's chunk) */
constexpr uint32_t IT_RUN = 1u << 28;   /* queued during a chunk's run-over */
constexpr uint32_t IT_OUT = 1u << 29;   /* report the outputs of the state itself at pos */
/* with IT_RUN | IT_CONT: the lane stopped its run-over in this state (it has a row) after k steps;
 * walk on from it with no hotfail bound (walk_continuation) */
constexpr uint32_t IT_WALK = 1u << 30;

/* Whether a record breaks the contract of the calls that take a record set: its end lies outside [pos_base,
 * pos_base + n_symbols), its length is 0, or it begins in front of pos_base.  Such a record is skipped and the
 * plan's error flag raised (select's rule). */
__device__ __forceinline__ bool
record_breaks_contract (uint64_t pos, uint32_t length, uint64_t pos_base, uint64_t n_symbols) {
  return pos < pos_base || pos - pos_base >= n_symbols || length == 0 || (uint64_t)length - 1 > pos - pos_base;
}

/* The joins of a record set under a compiled set (PATTERNS, CHAINS, APPROX and what runs APPROX's passes): control
 * words at the head of the passes' scratch, cleared in front of every call ... */
struct JoinCtl {
  unsigned long long n; /* records the passes work on (0 after an overflow and under bad offsets) */
  unsigned int bad;     /* offsets[] break the batch contract (offsets_check_kernel): nothing matches */
  unsigned int pad;
};

/* ... and the head of their kernel arguments: PatternsK, ChainsK and ApproxK derive from it and add the compiled set
 * and what their passes alone need */
struct JoinK {
  const ACMRecord *in;             /* canonical order */
  uint64_t capacity;               /* of `in`; the count itself when n_dev is NULL */
  const unsigned long long *n_dev; /* the record count (device), or NULL */
  uint64_t n_symbols, pos_base;
  const uint64_t *offsets;         /* [n_texts + 1], NULL: one text */
  uint64_t n_texts;
  uint32_t tile;                   /* records per tile, a multiple of WAVE */
  uint64_t n_tiles;                /* tiles of `capacity` records */
  unsigned long long *count;       /* [capacity + 1] matches per record (the last entry stays 0) */
  const unsigned long long *first; /* [capacity + 1] their exclusive prefix sum: [capacity] = all matches */
  ACMRecord *out;
  uint64_t out_capacity;
  unsigned long long *d_count;
  JoinCtl *ctl;
  unsigned int *error; /* the plan's device-side flag (acm_gpu_plan_status) */
};

/* The postings [begin, end) of record r's keyword in a set's index post_ptr[n_keywords + 1]; a record that breaks
 * the contract sets `bad` (which is never cleared here: callers gather it over their records) and has no posting,
 * and neither has a keyword the plan got after the set was made.  (CHAINS, whose bad records keep their postings,
 * has a form of its own: chains_postings.) */
__device__ __forceinline__ void
join_postings (const JoinK &K, const uint32_t *post_ptr, uint32_t n_keywords, const uint4 r, uint32_t &begin, uint32_t &end, bool &bad) {
  begin = end = 0;
  if (record_breaks_contract (((uint64_t)r.y << 32) | r.x, r.z, K.pos_base, K.n_symbols)) {
    bad = true;
    return;
  }
  if (r.w < n_keywords) {
    begin = post_ptr[r.w];
    end = post_ptr[r.w + 1];
  }
}

#include "dev_emit.h"
#include "dev_dense.h"
#include "dev_csr.h"
#include "dev_sparse.h"
#include "dev_starts.h"
#include "dev_gram.h"
#include "dev_gram2.h"
#include "dev_short.h"
#include "dev_misc.h"
#include "dev_order.h"
#include "dev_tiles.h"
#include "dev_batch.h"
#include "dev_flows.h"
#include "dev_tally.h"
#include "dev_select.h"
#include "dev_replace.h"
#include "dev_tokens.h"
#include "dev_grep.h"
#include "dev_tally_batch.h"
#include "dev_rules.h"
#include "dev_split.h"
#include "dev_words.h"
#include "dev_context.h"
#include "dev_anchored.h"
#include "dev_patterns.h"
#include "dev_approx.h"
#include "dev_templates.h"
#include "dev_edit.h"
#include "dev_chains.h"
#include "dev_near.h"
#include "dev_segment.h"
#include "dev_score.h"
#include "dev_index.h"
#include "dev_cooccur.h"
#include "dev_chars.h"

static_assert (WORDS_THREADS == OFFSETS_CHECK_THREADS && CONTEXT_THREADS == OFFSETS_CHECK_THREADS && ANCHORED_THREADS == OFFSETS_CHECK_THREADS &&
                 PATTERNS_THREADS == OFFSETS_CHECK_THREADS && APPROX_THREADS == OFFSETS_CHECK_THREADS && CHARS_THREADS == OFFSETS_CHECK_THREADS,
               "offsets_check_kernel is launched with the block of the family it checks for");

} // namespace
