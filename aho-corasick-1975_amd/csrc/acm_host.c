/*
 * acm_host.c -- host side of the drop-in: the acm_* API of include/acm.h.
 *
 * Own design, same observable behaviour as /root/reference/aho_corasick.c:
 *   - states live in slab arenas (stable addresses: an ACState* is the caller's cursor);
 *   - a state's goto edges are a comparator-ordered vector of child pointers (each child carries
 *     the letter of its incoming edge), searched by bisection -- the role minimaps' ordered map
 *     plays at aho_corasick.c:175,299;
 *   - failure links, output counts and the inverse failure sets are kept exact after EVERY
 *     inserted symbol (Meyer 1985, the reference's default build, aho_corasick.c:194-267,318-363),
 *     so matching and insertion interleave freely (generic_test.c:198-229);
 *   - every terminal state also records its first-insertion rank (keyword_id of acm_gpu.h) and
 *     every state its depth, which the flattener (acm_flat.c) ships to the GPU.
 *
 * -DACM_NMEYER_85 (the reference's -DNMEYER_85 build, aho_corasick.c:365-418,443-446; Makefile
 * target `nmeyer85` -> libac75_amd_nmeyer85.so): no incremental maintenance; inserting only marks
 * the failure function stale, and the next acm_match (or flatten, or acm_print) recomputes it for
 * the whole trie by the breadth-first pass of Aho & Corasick 1975, algorithm 3.  The automaton is
 * the same, so the flat tables and every scan are too (tests/test_nmeyer85.py).
 */
#define _GNU_SOURCE
#include "acm_internal.h"

#include <stdlib.h>
#include <string.h>
#include <threads.h>

/* reference error convention, aho_corasick.c:24-36: message on stderr, the calling THREAD exits. */
#define ACM_REQUIRE(cond, msg)                                                                      \
  do {                                                                                              \
    if (!(cond)) {                                                                                  \
      fflush (stdout);                                                                              \
      fprintf (stderr, "FATAL ERROR: A prerequisite is not fulfilled in function %s.\n", __func__); \
      fprintf (stderr, "             %s\n", (msg)[0] ? (msg) : "The condition (" #cond ") is false."); \
      thrd_exit (EXIT_FAILURE);                                                                     \
    }                                                                                               \
  } while (0)

#define SLAB_STATES 4096

struct slab {
  struct slab *next;
  uint32_t used;
  struct _ac_state states[SLAB_STATES];
};

/* an outgrown block kept until acm_release (blocks double, so all of them together are smaller
 * than the live ones) */
struct garbage {
  struct garbage *next;
  void *block;
};

struct _ac_machine {
  struct _ac_state *root;
  size_t nb_keywords;
  uint32_t nb_states;
  uint64_t generation;
  CMP_TYPE cmp;
  void *cmp_arg;
  DESTROY_TYPE letter_dtor;
  struct slab *slabs;
  mtx_t lock;
  mtx_t plan_lock; /* users of the cached device plan (acm_scan), one at a time */
  void *plan; /* cached device plan, see acm_gpu.hip */
  struct garbage *garbage; /* outgrown edge blocks: lock-free readers may still hold them */
  struct _ac_state **keywords; /* keyword_id -> terminal state (acm_get_keyword) */
  size_t keywords_cap;
  int stale; /* ACM_NMEYER_85: failure links and output counts await the breadth-first pass */
  uint32_t declared_sym_bytes; /* acm_set_symbol_bytes: symbol size of a machine with a comparator of its own (0: not said) */
  int scan_path;               /* acm_scan_path: what the last acm_scan on this machine ran */
};

void (*acm_internal_plan_dropper) (void *plan) = 0;

/* ------------------------------------------------------------------ default comparator */
static int
cmp_bytes (const void *a, const void *b, const void *arg) { /* reference :134-138 */
  return memcmp (a, b, *(const size_t *)arg);
}
const CMP_TYPE ACM_CMP_DEFAULT = cmp_bytes;
#ifdef ACM_NMEYER_85
const int ACM_INCREMENTAL_STRING_MATCHING = 0; /* reference :596-597 */
#else
const int ACM_INCREMENTAL_STRING_MATCHING = 1; /* reference :596-597 (default build) */
#endif

/* ------------------------------------------------------------------ internal accessors */
uint64_t
acm_internal_generation (const ACMachine *m) {
  return m->generation;
}
ACState *
acm_internal_root (const ACMachine *m) {
  return m->root;
}
uint32_t
acm_internal_nb_states (const ACMachine *m) {
  return m->nb_states;
}
int
acm_internal_symbol_bytes (const ACMachine *m, uint32_t *sym_bytes) {
  if (m->cmp != ACM_CMP_DEFAULT || !m->cmp_arg)
    return ACM_GPU_E_INELIGIBLE;
  size_t sz = *(const size_t *)m->cmp_arg;
  if (sz != 1 && sz != 2 && sz != 4 && sz != 8)
    return ACM_GPU_E_INELIGIBLE;
  *sym_bytes = (uint32_t)sz;
  return ACM_GPU_OK;
}
/* include/acm_gpu.h: the symbol size of a machine whose comparator is not ACM_CMP_DEFAULT (the
 * library cannot know it: letters are opaque pointers, aho_corasick.h:33-43) -- what acm_scan
 * needs to step through a buffer */
int
acm_set_symbol_bytes (ACMachine *machine, uint32_t sym_bytes) {
  if (!machine || sym_bytes == 0 || sym_bytes > 4096)
    return ACM_GPU_E_ARG;
  uint32_t own = 0;
  if (acm_internal_symbol_bytes (machine, &own) == ACM_GPU_OK && own != sym_bytes)
    return ACM_GPU_E_ARG; /* ACM_CMP_DEFAULT says it itself */
  machine->declared_sym_bytes = sym_bytes;
  return ACM_GPU_OK;
}
uint32_t
acm_internal_declared_symbol_bytes (const ACMachine *m) {
  return m->declared_sym_bytes;
}
int
acm_scan_path (const ACMachine *machine) {
  return machine ? machine->scan_path : ACM_SCAN_PATH_NONE;
}
void
acm_internal_set_scan_path (ACMachine *m, int path) {
  m->scan_path = path;
}

void
acm_internal_comparator (const ACMachine *m, CMP_TYPE *cmp, void **cmp_arg) {
  *cmp = m->cmp;
  *cmp_arg = m->cmp_arg;
}
void
acm_internal_lock (ACMachine *m) {
  ACM_REQUIRE (mtx_lock (&m->lock) == thrd_success, "");
}
void
acm_internal_unlock (ACMachine *m) {
  ACM_REQUIRE (mtx_unlock (&m->lock) == thrd_success, "");
}
void
acm_internal_plan_lock (ACMachine *m) {
  ACM_REQUIRE (mtx_lock (&m->plan_lock) == thrd_success, "");
}
void
acm_internal_plan_unlock (ACMachine *m) {
  ACM_REQUIRE (mtx_unlock (&m->plan_lock) == thrd_success, "");
}
void **
acm_internal_plan_slot (ACMachine *m) {
  return &m->plan;
}

/* Readers (acm_match, acm_get_match) take no lock -- the reference's threading model: many
 * threads, one shared machine, one cursor per thread, insertions in between (README.md:364,
 * aho_corasick.c:81).  Writers hold the machine lock and publish with release stores; readers use
 * acquire loads of the fields a writer may change under them (fail, nb_outputs, terminal, the
 * edge block and its sequence lock). */
#define LOAD(p) __atomic_load_n ((p), __ATOMIC_ACQUIRE)
#define STORE(p, v) __atomic_store_n ((p), (v), __ATOMIC_RELEASE)

/* ------------------------------------------------------------------ states */
static struct _ac_state *
state_alloc (ACMachine *m) {
  struct slab *sl = m->slabs;
  if (!sl || sl->used == SLAB_STATES) {
    sl = malloc (sizeof *sl);
    ACM_REQUIRE (sl, "Out of memory.");
    sl->next = m->slabs;
    sl->used = 0;
    m->slabs = sl;
  }
  struct _ac_state *s = &sl->states[sl->used++];
  memset (s, 0, sizeof *s);
  s->machine = m;
  s->id = m->nb_states++;
  s->rank = UINT32_MAX;
  return s;
}

/* bisection among the children of s; *at = where a missing letter would be inserted.
 * Safe beside a writer: the snapshot is retried if an insertion into this very state ran
 * meanwhile (sequence lock), and a replaced block stays allocated. */
static inline struct _ac_state *
child_find (const struct _ac_state *s, const void *letter, uint32_t *at) {
  const ACMachine *m = s->machine;
  for (;;) {
    const uint32_t v0 = LOAD (&s->kver);
    if (v0 & 1u)
      continue; /* an insertion is shifting the entries right now */
    const struct _ac_kidvec *kv = LOAD (&s->kids);
    uint32_t lo = 0, hi = kv ? __atomic_load_n (&kv->n, __ATOMIC_RELAXED) : 0;
    struct _ac_state *found = 0;
    while (lo < hi) {
      uint32_t mid = lo + (hi - lo) / 2;
      struct _ac_state *k = LOAD (&kv->v[mid]);
      int c = m->cmp (letter, k->letter, m->cmp_arg);
      if (c == 0) {
        found = k;
        break;
      }
      if (c < 0)
        hi = mid;
      else
        lo = mid + 1;
    }
    __atomic_thread_fence (__ATOMIC_ACQUIRE);
    if (__atomic_load_n (&s->kver, __ATOMIC_RELAXED) != v0)
      continue;
    if (!found && at)
      *at = lo;
    return found;
  }
}

/* writer, machine lock held: child k goes to position `at` of n's edges */
static void
child_insert (struct _ac_state *n, uint32_t at, struct _ac_state *k) {
  ACMachine *m = n->machine;
  struct _ac_kidvec *kv = n->kids;
  const uint32_t cnt = kv ? kv->n : 0;
  if (!kv || cnt == kv->cap) {
    /* a fresh block, published whole; the old one goes to the machine's garbage */
    const uint32_t cap = cnt ? 2 * cnt : 2;
    struct _ac_kidvec *nv = malloc (sizeof *nv + cap * sizeof nv->v[0]);
    struct garbage *g = kv ? malloc (sizeof *g) : 0;
    ACM_REQUIRE (nv && (g || !kv), "Out of memory.");
    nv->cap = cap;
    nv->n = cnt + 1;
    if (at)
      memcpy (nv->v, kv->v, at * sizeof nv->v[0]);
    nv->v[at] = k;
    if (cnt > at)
      memcpy (nv->v + at + 1, kv->v + at, (cnt - at) * sizeof nv->v[0]);
    STORE (&n->kids, nv);
    if (kv) {
      g->block = kv;
      g->next = m->garbage;
      m->garbage = g;
    }
    return;
  }
  __atomic_store_n (&n->kver, n->kver + 1, __ATOMIC_RELAXED); /* odd: readers wait */
  __atomic_thread_fence (__ATOMIC_RELEASE);
  for (uint32_t i = cnt; i > at; i--)
    __atomic_store_n (&kv->v[i], kv->v[i - 1], __ATOMIC_RELAXED);
  STORE (&kv->v[at], k);
  __atomic_store_n (&kv->n, cnt + 1, __ATOMIC_RELAXED);
  STORE (&n->kver, n->kver + 1);
}

/* delta(s, letter) of the automaton WITHOUT root self-loops: goto if defined, else down the
 * failure chain; a miss at the root stays there (reference state_goto, :167-192). */
static inline const struct _ac_state *
automaton_step (const struct _ac_state *s, const void *letter) {
  for (;;) {
    const struct _ac_state *k = child_find (s, letter, 0);
    if (k)
      return k;
    const struct _ac_state *f = LOAD (&s->fail);
    if (!f) /* only the root has no failure link */
      return s;
    s = f;
  }
}

static void
inv_add (struct _ac_state *owner, struct _ac_state *x) {
  if (owner->ninv == owner->capinv) {
    owner->capinv = owner->capinv ? 2 * owner->capinv : 4;
    owner->inv = realloc (owner->inv, owner->capinv * sizeof *owner->inv);
    ACM_REQUIRE (owner->inv, "Out of memory.");
  }
  x->inv_slot = owner->ninv;
  owner->inv[owner->ninv++] = x;
}

static void
inv_del (struct _ac_state *owner, struct _ac_state *x) {
  struct _ac_state *last = owner->inv[--owner->ninv];
  owner->inv[x->inv_slot] = last;
  last->inv_slot = x->inv_slot;
}

/* explicit stack for walks over the failure tree (depth can reach the number of states) */
struct walk {
  struct _ac_state **v;
  size_t n, cap;
};
static inline void
walk_push (struct walk *w, struct _ac_state *s) {
  if (w->n == w->cap) {
    w->cap = w->cap ? 2 * w->cap : 64;
    w->v = realloc (w->v, w->cap * sizeof *w->v);
    ACM_REQUIRE (w->v, "Out of memory.");
  }
  w->v[w->n++] = s;
}

/* New leaf `leaf` = child of n on letter c, about to be linked into the goto tree (it becomes
 * reachable only afterwards, complete: child_insert).
 * Failure maintenance (Meyer 1985; reference :194-208, :211-239, :253-265):
 *   f(leaf) = delta(f(n), c), or the root when n is the root;
 *   every existing node x.c whose longest proper suffix in the trie has just become `leaf` is
 *   re-pointed: those are the c-children of the nodes x met by a walk down the failure tree from
 *   n that stops at the first node owning a c-child on each branch.
 * The walk runs on the tree as it was BEFORE any re-pointing (targets are collected first), so
 * it does not depend on container mutation order. */
#ifdef ACM_NMEYER_85
__attribute__ ((unused))
#endif
static void
link_failure_of_new_leaf (struct _ac_state *n, struct _ac_state *leaf) {
  if (n->fail)
    leaf->fail = (struct _ac_state *)automaton_step (n->fail, leaf->letter);
  else
    leaf->fail = n; /* depth-1 states fail to the root */
  leaf->nb_outputs = leaf->fail->nb_outputs; /* leaf is not (yet) a keyword end */

  if (n->ninv) {
    struct walk todo = { 0 }, hits = { 0 };
    for (uint32_t i = 0; i < n->ninv; i++)
      walk_push (&todo, n->inv[i]);
    while (todo.n) {
      struct _ac_state *x = todo.v[--todo.n];
      struct _ac_state *xc = child_find (x, leaf->letter, 0);
      if (xc)
        walk_push (&hits, xc);
      else
        for (uint32_t i = 0; i < x->ninv; i++)
          walk_push (&todo, x->inv[i]);
    }
    for (size_t i = 0; i < hits.n; i++) {
      struct _ac_state *xc = hits.v[i];
      /* old f(xc) == f(leaf): both are the longest suffix shorter than leaf, so nb_outputs(xc)
       * is unchanged by the re-pointing. */
      inv_del (xc->fail, xc);
      STORE (&xc->fail, leaf);
      inv_add (leaf, xc);
    }
    free (todo.v);
    free (hits.v);
  }
  inv_add (leaf->fail, leaf);
}

/* AC-75, algorithm 3 (reference :365-418): failure links and output counts of the whole trie in
 * one breadth-first pass -- f of a depth-1 state is the root; f(child of u on a) = the first goto
 * on a met down u's failure chain, else the root; nb_outputs(s) = [s terminal] + nb_outputs(f(s)).
 * Does nothing in the default (Meyer-85) build, whose links are always current. */
void
acm_internal_refresh (ACMachine *m) {
#ifdef ACM_NMEYER_85
  if (!LOAD (&m->stale))
    return;
  ACM_REQUIRE (mtx_lock (&m->lock) == thrd_success, "");
  if (m->stale) {
    struct _ac_state **queue = malloc ((size_t)m->nb_states * sizeof *queue);
    ACM_REQUIRE (queue, "Out of memory.");
    size_t head = 0, tail = 0;
    queue[tail++] = m->root;
    while (head < tail) {
      struct _ac_state *u = queue[head++];
      for (uint32_t i = 0; i < ACM_NKIDS (u); i++) {
        struct _ac_state *c = ACM_KID (u, i), *target = m->root;
        for (const struct _ac_state *v = u->fail; v; v = v->fail) {
          struct _ac_state *t = child_find (v, c->letter, 0);
          if (t) {
            target = t;
            break;
          }
        }
        STORE (&c->fail, target);
        STORE (&c->nb_outputs, (uint32_t)(c->terminal ? 1 : 0) + target->nb_outputs);
        queue[tail++] = c;
      }
    }
    free (queue);
    STORE (&m->stale, 0);
  }
  ACM_REQUIRE (mtx_unlock (&m->lock) == thrd_success, "");
#else
  (void)m;
#endif
}

/* ------------------------------------------------------------------ public API */
ACMachine *
acm_create (CMP_TYPE cmp, void *cmp_arg, DESTROY_TYPE dtor) {
  ACM_REQUIRE (cmp, "A comparison function should be provided.");
  ACMachine *m = calloc (1, sizeof *m);
  ACM_REQUIRE (m, "Out of memory.");
  m->cmp = cmp;
  m->cmp_arg = cmp_arg;
  m->letter_dtor = dtor;
  m->root = state_alloc (m);
  ACM_REQUIRE (mtx_init (&m->lock, mtx_plain) == thrd_success, "Out of memory.");
  ACM_REQUIRE (mtx_init (&m->plan_lock, mtx_plain) == thrd_success, "Out of memory.");
  return m;
}

void
acm_release (ACMachine *machine) {
  ACM_REQUIRE (machine, "Invalid null machine.");
  if (machine->plan && acm_internal_plan_dropper)
    acm_internal_plan_dropper (machine->plan);
  for (struct slab *sl = machine->slabs; sl;) {
    for (uint32_t i = 0; i < sl->used; i++) {
      struct _ac_state *s = &sl->states[i];
      if (s->parent && machine->letter_dtor) /* stored letters, reference :111-112 */
        machine->letter_dtor (s->letter);
      if (s->value_dtor) /* reference :124-125 */
        s->value_dtor (s->value);
      free (s->kids);
      free (s->inv);
    }
    struct slab *next = sl->next;
    free (sl);
    sl = next;
  }
  for (struct garbage *g = machine->garbage; g;) {
    struct garbage *next = g->next;
    free (g->block);
    free (g);
    g = next;
  }
  mtx_destroy (&machine->lock);
  mtx_destroy (&machine->plan_lock);
  free (machine->keywords);
  free (machine);
}

ACState *
acm_initiate (ACMachine *machine) {
  ACM_REQUIRE (machine, "Invalid null machine.");
  return machine->root;
}

void
acm_insert_letter_of_keyword (ACState **state, void *letter) {
  ACM_REQUIRE (state && *state && letter, "Invalid null state or letter.");
  struct _ac_state *n = *state;
  ACMachine *m = n->machine;
  ACM_REQUIRE (mtx_lock (&m->lock) == thrd_success, "");
  uint32_t at = 0;
  struct _ac_state *k = child_find (n, letter, &at);
  if (k) {
    if (m->letter_dtor) /* the edge exists: this copy of the letter is not kept, reference :306-307 */
      m->letter_dtor (letter);
  } else {
    k = state_alloc (m);
    k->parent = n;
    k->letter = letter;
    k->depth = n->depth + 1;
#ifdef ACM_NMEYER_85
    k->fail = m->root; /* provisional (only the root may have none): acm_internal_refresh sets it */
    m->stale = 1;
#else
    link_failure_of_new_leaf (n, k);
#endif
    child_insert (n, at, k);
    m->generation++;
  }
  *state = k;
  ACM_REQUIRE (mtx_unlock (&m->lock) == thrd_success, "");
}

void *
acm_insert_end_of_keyword (ACState **state, void *value, void (*dtor) (void *)) {
  ACM_REQUIRE (state && *state, "Invalid null state.");
  struct _ac_state *n = *state;
  ACMachine *m = n->machine;
  ACM_REQUIRE (mtx_lock (&m->lock) == thrd_success, "");
  ACM_REQUIRE (n != m->root, "acm_insert_letter_of_keyword should be called first.");
  void *previous = n->value;
  if (!previous) { /* first non-NULL value wins, reference :357-359 */
    n->value_dtor = dtor;
    if (value)
      STORE (&n->value, value);
  }
  if (!n->terminal) {
    if (m->nb_keywords == m->keywords_cap) {
      m->keywords_cap = m->keywords_cap ? 2 * m->keywords_cap : 64;
      m->keywords = realloc (m->keywords, m->keywords_cap * sizeof *m->keywords);
      ACM_REQUIRE (m->keywords, "Out of memory.");
    }
    m->keywords[m->nb_keywords] = n;
    n->rank = (uint32_t)m->nb_keywords++;
    /* the terminal mark first, then the counts: a reader that sees a count sees the terminal
     * states acm_get_match will look for down the failure chain */
    STORE (&n->terminal, 1);
#ifdef ACM_NMEYER_85
    m->stale = 1; /* the output counts come with the next breadth-first pass */
    if (0) {
#else
    {
#endif
    /* one more keyword ends at n and at every state that has n as a suffix, i.e. the whole
     * failure subtree of n (reference enter_output, :330-338) */
    struct walk todo = { 0 };
    walk_push (&todo, n);
    while (todo.n) {
      struct _ac_state *x = todo.v[--todo.n];
      STORE (&x->nb_outputs, x->nb_outputs + 1);
      for (uint32_t i = 0; i < x->ninv; i++)
        walk_push (&todo, x->inv[i]);
    }
    free (todo.v);
    }
    m->generation++;
  }
  *state = m->root;
  ACM_REQUIRE (mtx_unlock (&m->lock) == thrd_success, "");
  return previous;
}

size_t
acm_match (const ACState **state, const void *letter) {
  ACM_REQUIRE (state && *state && letter, "Invalid null state or letter.");
#ifdef ACM_NMEYER_85
  acm_internal_refresh ((*state)->machine); /* reference :443-446 */
#endif
  return LOAD (&(*state = automaton_step (*state, letter))->nb_outputs);
}

void
acm_matcher_init (MatchHolder *matcher) {
  ACM_REQUIRE (matcher, "Invalid null matcher.");
  matcher->letters = 0;
  matcher->length = 0;
  matcher->value = 0;
}

void
acm_matcher_release (MatchHolder *matcher) {
  ACM_REQUIRE (matcher, "Invalid null matcher.");
  free (matcher->letters);
  acm_matcher_init (matcher);
}

void
acm_get_match (const ACState *state, size_t index, MatchHolder *matcher) {
  ACM_REQUIRE (state, "Invalid null state.");
  ACM_REQUIRE (state->parent, "acm_match should be called first and acm_matcher_init called on the MatchHolder.");
  ACM_REQUIRE (index < LOAD (&state->nb_outputs), "Index out of bounds.");
  /* index-th keyword-terminal state along the failure chain, nearest (= longest) first
   * (reference :459-466) */
  const struct _ac_state *t = state;
  for (size_t seen = 0;; t = LOAD (&t->fail)) {
    if (LOAD (&t->terminal) && seen++ == index)
      break;
  }
  if (!matcher)
    return;
  matcher->length = t->depth;
  matcher->letters = realloc (matcher->letters, matcher->length * sizeof *matcher->letters);
  ACM_REQUIRE (matcher->letters || !matcher->length, "Out of memory.");
  size_t k = matcher->length;
  for (const struct _ac_state *s = t; s->parent; s = s->parent)
    matcher->letters[--k] = s->letter;
  matcher->value = LOAD (&t->value);
}

/* What acm_get_match would have put into the holder for a record of the bulk scan: the
 * dictionary's letters, the length and the value of keyword `keyword_id` (include/acm_gpu.h). */
int
acm_get_keyword (const ACMachine *machine, uint32_t keyword_id, MatchHolder *matcher) {
  if (!machine || !matcher)
    return ACM_GPU_E_ARG;
  /* the keyword table may be moved by a concurrent acm_insert_end_of_keyword */
  ACMachine *m = (ACMachine *)machine;
  acm_internal_lock (m);
  const int rc = acm_internal_get_keyword (machine, keyword_id, matcher);
  acm_internal_unlock (m);
  return rc;
}

int
acm_internal_get_keyword (const ACMachine *machine, uint32_t keyword_id, MatchHolder *matcher) {
  if (!machine || !matcher || keyword_id >= machine->nb_keywords)
    return ACM_GPU_E_ARG;
  const struct _ac_state *t = machine->keywords[keyword_id];
  matcher->length = t->depth;
  matcher->letters = realloc (matcher->letters, matcher->length * sizeof *matcher->letters);
  if (!matcher->letters && matcher->length)
    return ACM_GPU_E_NOMEM;
  size_t k = matcher->length;
  for (const struct _ac_state *s = t; s->parent; s = s->parent)
    matcher->letters[--k] = s->letter;
  matcher->value = t->value;
  return ACM_GPU_OK;
}

size_t
acm_nb_keywords (const ACMachine *machine) {
  ACM_REQUIRE (machine, "Invalid null machine.");
  return machine->nb_keywords;
}

/* ------------------------------------------------------------------ enumeration / debug */
struct dfs_frame {
  const struct _ac_state *s;
  uint32_t next_kid;
};

void
acm_foreach_keyword (const ACMachine *machine, void (*operator_) (MatchHolder)) {
  ACM_REQUIRE (machine, "Invalid null machine.");
  if (!operator_)
    return;
  /* iterative pre-order DFS in comparator order (reference :490-519) */
  size_t cap = 16, top = 0;
  struct dfs_frame *st = malloc (cap * sizeof *st);
  const void **letters = malloc (cap * sizeof *letters);
  ACM_REQUIRE (st && letters, "Out of memory.");
  st[top++] = (struct dfs_frame){ machine->root, 0 };
  while (top) {
    struct dfs_frame *f = &st[top - 1];
    if (f->next_kid == 0 && f->s->terminal && f->s->depth) {
      MatchHolder k = { .letters = letters, .length = f->s->depth, .value = f->s->value };
      operator_ (k);
    }
    if (f->next_kid < ACM_NKIDS (f->s)) {
      const struct _ac_state *kid = ACM_KID (f->s, f->next_kid++);
      if (top == cap) {
        cap *= 2;
        st = realloc (st, cap * sizeof *st);
        letters = realloc (letters, cap * sizeof *letters);
        ACM_REQUIRE (st && letters, "Out of memory.");
      }
      letters[kid->depth - 1] = kid->letter;
      st[top++] = (struct dfs_frame){ kid, 0 };
    } else
      top--;
  }
  free (st);
  free (letters);
}

/* Tree drawing, same text as the reference's (:541-594): one edge is
 *   ---<letter>-->(<id>)[+<outputs> if keyword end](v <fail id> if the failure link is not the root)
 * the root id is printed in front of each of its edges; the first child continues the line, the
 * next ones start a new line indented to their parent's column with an 'L' elbow. */
static void
print_subtree (const struct _ac_state *s, FILE *out, int *col, int indent, PRINT_TYPE printer) {
  for (uint32_t i = 0; i < ACM_NKIDS (s); i++) {
    const struct _ac_state *k = ACM_KID (s, i);
    if (indent < *col) {
      *col = 0;
      fprintf (out, "\n");
      if (indent) {
        for (int t = 0; t < indent - 1; t++)
          *col += fprintf (out, " ");
        *col += fprintf (out, "L");
      }
    } else
      while (*col < indent)
        *col += fprintf (out, " ");
    if (!s->parent)
      *col += fprintf (out, "(%03zu)", (size_t)s->id);
    *col += fprintf (out, "---");
    if (printer)
      *col += printer (out, k->letter);
    *col += fprintf (out, "-->(%03zu)", (size_t)k->id);
    if (k->terminal)
      *col += fprintf (out, "[+%zu]", (size_t)k->nb_outputs);
    if (k->fail != s->machine->root)
      *col += fprintf (out, "(v %03zu)", (size_t)k->fail->id);
    print_subtree (k, out, col, *col, printer);
  }
}

void
acm_print (ACMachine *machine, FILE *stream, PRINT_TYPE printer) {
  ACM_REQUIRE (machine, "Invalid null machine.");
  acm_internal_refresh (machine); /* reference :589: also with a null stream */
  if (!stream)
    return;
  int col = 0;
  fprintf (stream, "\n");
  print_subtree (machine->root, stream, &col, 0, printer);
  fprintf (stream, "\n");
}

/* the caller loop over symbols [begin, end) of `text`, from *state (NULL: from the root); appends
 * behind the `found` records there are and returns the new total (text_id, when given, takes `id`
 * beside every record); *state becomes the state the loop ends in */
static uint64_t
cpu_loop_from (const ACMachine *m, const struct _ac_state **state, const void *text, uint64_t begin, uint64_t end, uint32_t sym_bytes,
               ACMRecord *records, uint32_t *text_id, uint32_t id, uint64_t capacity, uint64_t found) {
  const unsigned char *t = text;
  const struct _ac_state *s = state && *state ? *state : m->root;
  for (uint64_t i = begin; i < end; i++) {
    s = automaton_step (s, t + i * sym_bytes);
    uint32_t nb = LOAD (&s->nb_outputs);
    for (const struct _ac_state *o = s; nb; o = LOAD (&o->fail)) { /* nearest (= longest) terminal state first */
      if (!LOAD (&o->terminal))
        continue;
      if (found < capacity) {
        records[found].end_pos = i;
        records[found].length = o->depth;
        records[found].keyword_id = o->rank;
        if (text_id)
          text_id[found] = id;
      }
      found++;
      nb--;
    }
  }
  if (state)
    *state = s;
  return found;
}

static uint64_t
cpu_loop (const ACMachine *m, const void *text, uint64_t begin, uint64_t end, uint32_t sym_bytes, ACMRecord *records, uint32_t *text_id, uint32_t id,
          uint64_t capacity, uint64_t found) {
  return cpu_loop_from (m, NULL, text, begin, end, sym_bytes, records, text_id, id, capacity, found);
}

/* The reference's caller loop (examples/test.c:17-23; acm_match aho_corasick.c:434-448, acm_get_match
 * :451-482) over a buffer of fixed-size symbols, with THIS library's own automaton step and failure
 * chain -- what acm_scan runs for a machine the GPU path cannot take (a comparator of its own over
 * symbols that are not 1, 2 or 4 bytes wide, or one that is no consistent order over all values:
 * SURVEY.md 8b).  Records in the loop's order; *n_found = their total, also beyond `capacity`. */
int
acm_internal_cpu_scan (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records, uint64_t capacity,
                       uint64_t *n_found) {
  if (!m || !n_found || (n_symbols && !text) || (capacity && !records) || !sym_bytes)
    return ACM_GPU_E_ARG;
#ifdef ACM_NMEYER_85
  acm_internal_refresh (m);
#endif
  *n_found = cpu_loop (m, text, 0, n_symbols, sym_bytes, records, NULL, 0, capacity, 0);
  return *n_found > capacity ? ACM_GPU_E_OVERFLOW : ACM_GPU_OK;
}

/* The same loop over a batch (acm_scan_batch, include/acm_gpu.h): from the root at every offset,
 * end_pos = the index in the whole buffer; text_id and first may be NULL.  offsets[] has been
 * checked by the caller. */
int
acm_internal_cpu_scan_batch (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, ACMRecord *records,
                             uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  if (!m || !n_found || !offsets || (offsets[n_texts] && !text) || (capacity && !records) || !sym_bytes)
    return ACM_GPU_E_ARG;
#ifdef ACM_NMEYER_85
  acm_internal_refresh (m);
#endif
  uint64_t found = 0;
  for (uint64_t t = 0; t < n_texts; t++) {
    if (first)
      first[t] = found;
    found = cpu_loop (m, text, offsets[t], offsets[t + 1], sym_bytes, records, text_id, (uint32_t)t, capacity, found);
  }
  if (first)
    first[n_texts] = found;
  *n_found = found;
  return found > capacity ? ACM_GPU_E_OVERFLOW : ACM_GPU_OK;
}

/* The same loop continued from *cursor (acm_scan_from, include/acm_gpu.h): end_pos = the index in
 * `text`; *cursor becomes the state the loop ends in, and stays as it is when the records do not fit. */
int
acm_internal_cpu_scan_from (ACMachine *m, const ACState **cursor, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records,
                            uint64_t capacity, uint64_t *n_found) {
  if (!m || !cursor || !*cursor || !n_found || (n_symbols && !text) || (capacity && !records) || !sym_bytes)
    return ACM_GPU_E_ARG;
#ifdef ACM_NMEYER_85
  acm_internal_refresh (m);
#endif
  const struct _ac_state *s = *cursor;
  *n_found = cpu_loop_from (m, &s, text, 0, n_symbols, sym_bytes, records, NULL, 0, capacity, 0);
  if (*n_found > capacity)
    return ACM_GPU_E_OVERFLOW;
  *cursor = s;
  return ACM_GPU_OK;
}

/* The same loop for acm_tally (include/acm_gpu.h): what the reference's second example does with its
 * matches (examples/aho_corasick_generic_test.c:168-210, `(*(size_t *) m3.value)++`), per keyword id. */
int
acm_internal_cpu_tally (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t *tally, uint64_t n_keywords,
                        uint64_t *total) {
  if (!m || !tally || (n_symbols && !text) || !sym_bytes || n_keywords < acm_nb_keywords (m))
    return ACM_GPU_E_ARG;
#ifdef ACM_NMEYER_85
  acm_internal_refresh (m);
#endif
  const unsigned char *t = text;
  const struct _ac_state *s = m->root;
  uint64_t found = 0;
  for (uint64_t i = 0; i < n_symbols; i++) {
    s = automaton_step (s, t + i * sym_bytes);
    uint32_t nb = LOAD (&s->nb_outputs);
    for (const struct _ac_state *o = s; nb; o = LOAD (&o->fail)) {
      if (!LOAD (&o->terminal))
        continue;
      if (o->rank < n_keywords) /* (a keyword inserted by another thread since the check above is not counted) */
        tally[o->rank]++, found++;
      nb--;
    }
  }
  if (total)
    *total = found;
  return ACM_GPU_OK;
}

/* The same loop for acm_grep (include/acm_gpu.h): from the root at every offset, counting the matches
 * of every text -- the reference's word-by-word use (examples/aho_corasick_generic_test.c:168-210
 * restarts from acm_initiate for every word it reads).  offsets[] has been checked by the caller. */
int
acm_internal_cpu_grep_hits (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint64_t *hits) {
  if (!m || !offsets || (n_texts && !hits) || (offsets[n_texts] && !text) || !sym_bytes)
    return ACM_GPU_E_ARG;
#ifdef ACM_NMEYER_85
  acm_internal_refresh (m);
#endif
  for (uint64_t t = 0; t < n_texts; t++)
    hits[t] = cpu_loop (m, text, offsets[t], offsets[t + 1], sym_bytes, NULL, NULL, 0, 0, 0);
  return ACM_GPU_OK;
}

/* KEPT and GATHER of a batch under its hit counts (include/acm_gpu.h): the plain sequential pass.
 * The output is measured first, so that nothing is written to it when it has no room. */
int
acm_grep_gather (const void *text, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts, const uint64_t *hits, uint32_t flags,
                 uint32_t *kept, uint64_t *n_kept, void *out, uint64_t out_capacity, uint64_t *out_offsets, uint64_t *out_symbols) {
  if (!sym_bytes || !n_kept || !offsets || offsets[0] != 0 || (n_texts && !hits) || n_texts >= (1ull << 31) || flags > ACM_GREP_INVERT)
    return ACM_GPU_E_ARG;
  for (uint64_t t = 0; t < n_texts; t++)
    if (offsets[t] > offsets[t + 1])
      return ACM_GPU_E_ARG;
  if (out && offsets[n_texts] && !text)
    return ACM_GPU_E_ARG;
  const int invert = flags == ACM_GREP_INVERT;
  uint64_t k = 0, symbols = 0;
  for (uint64_t t = 0; t < n_texts; t++) {
    if ((hits[t] > 0) == invert)
      continue;
    if (kept)
      kept[k] = (uint32_t)t;
    if (out_offsets)
      out_offsets[k] = symbols;
    symbols += offsets[t + 1] - offsets[t];
    k++;
  }
  if (out_offsets)
    out_offsets[k] = symbols;
  *n_kept = k;
  if (out_symbols)
    *out_symbols = symbols;
  if (!out)
    return ACM_GPU_OK;
  if (symbols > out_capacity)
    return ACM_GPU_E_OVERFLOW;
  const unsigned char *src = text;
  unsigned char *o = out;
  const size_t sb = sym_bytes;
  uint64_t at = 0;
  for (uint64_t t = 0; t < n_texts; t++) {
    const uint64_t len = offsets[t + 1] - offsets[t];
    if ((hits[t] > 0) == invert || !len)
      continue;
    memcpy (o + at * sb, src + offsets[t] * sb, len * sb);
    at += len;
  }
  return ACM_GPU_OK;
}

/* SPLIT of a buffer at delimiter symbols (include/acm_gpu.h): the plain sequential pass.  The cuts
 * are counted first, so that nothing is written to offsets[] when it has no room. */
static int
split_is_delim (const unsigned char *sym, size_t sb, const unsigned char *delims, uint32_t n_delims) {
  for (uint32_t d = 0; d < n_delims; d++)
    if (memcmp (sym, delims + d * sb, sb) == 0)
      return 1;
  return 0;
}

int
acm_split_offsets (const void *text, uint64_t n_symbols, uint32_t sym_bytes, const void *delims, uint32_t n_delims, uint32_t flags, uint64_t *offsets,
                   uint64_t capacity, uint64_t *n_texts) {
  if (!sym_bytes || !n_texts || !delims || n_delims == 0 || n_delims > ACM_SPLIT_MAX_DELIMS || flags > ACM_SPLIT_RUNS || (n_symbols && !text))
    return ACM_GPU_E_ARG;
  const unsigned char *t = text;
  const size_t sb = sym_bytes;
  const int runs = flags == ACM_SPLIT_RUNS;
  for (int write = 0; write < 2; write++) {
    uint64_t k = 0;
    int here = n_symbols ? split_is_delim (t, sb, delims, n_delims) : 0;
    if (write)
      offsets[0] = 0;
    for (uint64_t i = 0; i < n_symbols; i++) {
      const int next = i + 1 < n_symbols ? split_is_delim (t + (i + 1) * sb, sb, delims, n_delims) : 0;
      if (i + 1 == n_symbols || (here && !(runs && next))) {
        k++;
        if (write)
          offsets[k] = i + 1;
      }
      here = next;
    }
    *n_texts = k;
    if (!offsets)
      break;
    if (k > capacity)
      return ACM_GPU_E_OVERFLOW;
  }
  return ACM_GPU_OK;
}

/* acm_grep_lines on the host (include/acm_gpu.h): the split, then acm_internal_cpu_grep over its
 * texts -- what ACM_SCAN_PATH_CPU_LOOP runs. */
int
acm_internal_cpu_grep_lines (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const void *delims, uint32_t n_delims,
                             uint32_t split_flags, uint32_t grep_flags, uint64_t *n_texts, uint64_t *n_kept, uint64_t *total, void *out,
                             uint64_t out_capacity, uint64_t *out_symbols, uint64_t texts_capacity, uint64_t *offsets, uint64_t *hits, uint32_t *kept,
                             uint64_t *out_offsets) {
  if (!m || !n_texts || !n_kept || grep_flags > ACM_GREP_INVERT)
    return ACM_GPU_E_ARG;
  uint64_t n = 0;
  int rc = acm_split_offsets (text, n_symbols, sym_bytes, delims, n_delims, split_flags, NULL, 0, &n);
  if (rc)
    return rc;
  *n_texts = n;
  if ((offsets || hits || kept || out_offsets) && n > texts_capacity)
    return ACM_GPU_E_OVERFLOW;
  if (n >= (1ull << 31))
    return ACM_GPU_E_ARG;
  uint64_t *own_off = offsets ? NULL : malloc ((n + 1) * sizeof (uint64_t));
  uint64_t *off = offsets ? offsets : own_off;
  if (!off)
    return ACM_GPU_E_NOMEM;
  rc = acm_split_offsets (text, n_symbols, sym_bytes, delims, n_delims, split_flags, off, n, &n);
  if (!rc)
    rc = acm_internal_cpu_grep (m, text, off, n, sym_bytes, grep_flags, hits, kept, n_kept, total, out, out_capacity, out_offsets, out_symbols);
  free (own_off);
  return rc;
}

static int
cmp_u32 (const void *a, const void *b) {
  const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
  return x < y ? -1 : x > y;
}

/* The text x keyword count matrix of a batch's records in CSR form (include/acm_gpu.h): the plain
 * sequential pass.  seen[k] = t + 1 while row t has met keyword k: the first walk counts every row's
 * distinct keywords, so that nothing is written to col and val when they have no room; the second
 * collects a row's keywords where they go, sorts them and reads their counters back (and clears
 * them). */
int
acm_tally_batch_records (const ACMRecord *records, const uint64_t *first, uint64_t n_texts, uint64_t n_keywords, uint64_t *row_ptr, uint32_t *col,
                         uint64_t *val, uint64_t nnz_capacity, uint64_t *nnz) {
  if (!first || first[0] != 0 || !row_ptr || !nnz || n_texts >= (1ull << 31) || n_keywords >= (1ull << 32))
    return ACM_GPU_E_ARG;
  for (uint64_t t = 0; t < n_texts; t++)
    if (first[t] > first[t + 1])
      return ACM_GPU_E_ARG;
  const uint64_t n = first[n_texts];
  if (n && !records)
    return ACM_GPU_E_ARG;
  for (uint64_t r = 0; r < n; r++)
    if (records[r].keyword_id >= n_keywords)
      return ACM_GPU_E_ARG;
  uint32_t *seen = calloc (n_keywords ? n_keywords : 1, sizeof (uint32_t));
  uint64_t *count = calloc (n_keywords ? n_keywords : 1, sizeof (uint64_t));
  if (!seen || !count) {
    free (seen);
    free (count);
    return ACM_GPU_E_NOMEM;
  }
  uint64_t all = 0;
  for (uint64_t t = 0; t < n_texts; t++) {
    row_ptr[t] = all;
    for (uint64_t r = first[t]; r < first[t + 1]; r++) {
      const uint32_t k = records[r].keyword_id;
      if (seen[k] != (uint32_t)t + 1) {
        seen[k] = (uint32_t)t + 1;
        all++;
      }
    }
  }
  row_ptr[n_texts] = all;
  *nnz = all;
  int rc = ACM_GPU_OK;
  if (col && val && all > nnz_capacity)
    rc = ACM_GPU_E_OVERFLOW;
  else if (col && val)
    for (uint64_t t = 0; t < n_texts; t++) {
      uint32_t *c = col + row_ptr[t];
      uint64_t m = 0;
      for (uint64_t r = first[t]; r < first[t + 1]; r++) {
        const uint32_t k = records[r].keyword_id;
        if (count[k]++ == 0)
          c[m++] = k;
      }
      qsort (c, m, sizeof (uint32_t), cmp_u32);
      for (uint64_t j = 0; j < m; j++) {
        val[row_ptr[t] + j] = count[c[j]];
        count[c[j]] = 0;
      }
    }
  free (seen);
  free (count);
  return rc;
}

/* The argument checks of a rule set (include/acm_gpu.h) */
int
acm_rules_check (const ACMRuleTerm *terms, const uint64_t *rule_ptr, const uint32_t *need, uint64_t n_rules, uint64_t n_keywords) {
  if (!rule_ptr || rule_ptr[0] != 0 || n_rules >= (1ull << 31) || (n_rules && (!terms || !need)))
    return ACM_GPU_E_ARG;
  for (uint64_t r = 0; r < n_rules; r++) {
    if (rule_ptr[r] >= rule_ptr[r + 1]) /* decreasing, or a rule without terms */
      return ACM_GPU_E_ARG;
    if (need[r] == 0 || need[r] > rule_ptr[r + 1] - rule_ptr[r])
      return ACM_GPU_E_ARG;
  }
  for (uint64_t i = 0; i < rule_ptr[n_rules]; i++)
    if (terms[i].keyword_id >= n_keywords || terms[i].lo > terms[i].hi)
      return ACM_GPU_E_ARG;
  return ACM_GPU_OK;
}

/* whether a term holds at count c */
static int
rule_term_holds (const ACMRuleTerm *term, uint64_t c) {
  return c >= term->lo && (term->hi == ACM_RULE_NO_MAX || c <= term->hi);
}

/* The text x rule matrix of a count matrix in CSR form (include/acm_gpu.h): the plain sequential
 * evaluation.  A row is spread into count[] (and taken back out), every rule looks its terms up
 * there; the first walk counts, so that nothing is written to `fired` when it has no room. */
int
acm_rules_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts, uint64_t n_keywords, const ACMRuleTerm *terms,
                  const uint64_t *rule_ptr, const uint32_t *need, uint64_t n_rules, uint64_t *fired_ptr, uint32_t *fired, uint64_t fired_capacity,
                  uint64_t *n_fired) {
  if (!row_ptr || row_ptr[0] != 0 || !fired_ptr || !n_fired || n_texts >= (1ull << 31) || n_keywords >= (1ull << 32))
    return ACM_GPU_E_ARG;
  if (acm_rules_check (terms, rule_ptr, need, n_rules, n_keywords))
    return ACM_GPU_E_ARG;
  for (uint64_t t = 0; t < n_texts; t++)
    if (row_ptr[t] > row_ptr[t + 1])
      return ACM_GPU_E_ARG;
  const uint64_t nnz = row_ptr[n_texts];
  if (nnz && (!col || !val))
    return ACM_GPU_E_ARG;
  for (uint64_t e = 0; e < nnz; e++)
    if (col[e] >= n_keywords)
      return ACM_GPU_E_ARG;
  uint64_t *count = calloc (n_keywords ? n_keywords : 1, sizeof (uint64_t));
  if (!count)
    return ACM_GPU_E_NOMEM;
  int rc = ACM_GPU_OK;
  for (int fill = 0; fill < 2 && !rc; fill++) {
    uint64_t all = 0;
    for (uint64_t t = 0; t < n_texts; t++) {
      if (!fill)
        fired_ptr[t] = all;
      for (uint64_t e = row_ptr[t]; e < row_ptr[t + 1]; e++)
        count[col[e]] += val[e];
      for (uint64_t r = 0; r < n_rules; r++) {
        uint64_t held = 0;
        for (uint64_t i = rule_ptr[r]; i < rule_ptr[r + 1]; i++)
          held += (uint64_t)rule_term_holds (&terms[i], count[terms[i].keyword_id]);
        if (held >= need[r]) {
          if (fill)
            fired[all] = (uint32_t)r;
          all++;
        }
      }
      for (uint64_t e = row_ptr[t]; e < row_ptr[t + 1]; e++)
        count[col[e]] = 0;
    }
    if (!fill) {
      fired_ptr[n_texts] = all;
      *n_fired = all;
      if (!fired)
        break; /* the call only counts */
      if (all > fired_capacity)
        rc = ACM_GPU_E_OVERFLOW;
    }
  }
  free (count);
  return rc;
}

/* The argument checks of a score model (include/acm_score.h) */
int
acm_score_check (const ACMScoreTerm *terms, const uint64_t *class_ptr, const int64_t *bias, const int64_t *threshold, uint64_t n_classes,
                 uint64_t n_keywords) {
  if (!class_ptr || class_ptr[0] != 0 || n_classes >= (1ull << 31) || (n_classes && (!bias || !threshold)))
    return ACM_GPU_E_ARG;
  for (uint64_t c = 0; c < n_classes; c++)
    if (class_ptr[c] > class_ptr[c + 1])
      return ACM_GPU_E_ARG;
  const uint64_t n_terms = class_ptr[n_classes];
  if (n_terms >= (1ull << 31) || (n_terms && !terms))
    return ACM_GPU_E_ARG;
  for (uint64_t i = 0; i < n_terms; i++)
    if (terms[i].keyword_id >= n_keywords || terms[i].cap == 0)
      return ACM_GPU_E_ARG;
  return ACM_GPU_OK;
}

/* a term's value at count c, modulo 2^64 */
static uint64_t
score_term_value (const ACMScoreTerm *term, uint64_t c) {
  const uint64_t capped = term->cap != ACM_SCORE_NO_CAP && c > term->cap ? term->cap : c;
  return (uint64_t)(int64_t)term->weight * capped;
}

/* The kept part of the text x class score matrix of a count matrix in CSR form (include/acm_score.h):
 * the plain sequential evaluation, acm_rules_matrix's walk with sums in place of held terms.  Sums are
 * unsigned, so that nothing overflows as a signed number; the first walk counts, so that nothing is
 * written to the kept entries or to best[] when they have no room. */
int
acm_score_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts, uint64_t n_keywords, const ACMScoreTerm *terms,
                  const uint64_t *class_ptr, const int64_t *bias, const int64_t *threshold, uint64_t n_classes, uint64_t *kept_ptr, uint32_t *kept_class,
                  int64_t *kept_score, uint64_t kept_capacity, uint64_t *n_kept, uint32_t *best) {
  if (!row_ptr || row_ptr[0] != 0 || !kept_ptr || !n_kept || n_texts >= (1ull << 31) || n_keywords >= (1ull << 32))
    return ACM_GPU_E_ARG;
  if (acm_score_check (terms, class_ptr, bias, threshold, n_classes, n_keywords))
    return ACM_GPU_E_ARG;
  for (uint64_t t = 0; t < n_texts; t++)
    if (row_ptr[t] > row_ptr[t + 1])
      return ACM_GPU_E_ARG;
  const uint64_t nnz = row_ptr[n_texts];
  if (nnz && (!col || !val))
    return ACM_GPU_E_ARG;
  for (uint64_t e = 0; e < nnz; e++)
    if (col[e] >= n_keywords)
      return ACM_GPU_E_ARG;
  uint64_t *count = calloc (n_keywords ? n_keywords : 1, sizeof (uint64_t));
  if (!count)
    return ACM_GPU_E_NOMEM;
  const int counts_only = !kept_class || !kept_score;
  int rc = ACM_GPU_OK;
  for (int fill = 0; fill < 2 && !rc; fill++) {
    uint64_t all = 0;
    for (uint64_t t = 0; t < n_texts; t++) {
      if (!fill)
        kept_ptr[t] = all;
      for (uint64_t e = row_ptr[t]; e < row_ptr[t + 1]; e++)
        count[col[e]] += val[e];
      uint32_t best_class = ACM_SCORE_NONE;
      int64_t best_score = 0;
      for (uint64_t c = 0; c < n_classes; c++) {
        uint64_t sum = (uint64_t)bias[c];
        for (uint64_t i = class_ptr[c]; i < class_ptr[c + 1]; i++)
          sum += score_term_value (&terms[i], count[terms[i].keyword_id]);
        const int64_t score = (int64_t)sum;
        if (score >= threshold[c]) {
          if (fill) {
            kept_class[all] = (uint32_t)c;
            kept_score[all] = score;
            if (best_class == ACM_SCORE_NONE || score > best_score) {
              best_class = (uint32_t)c;
              best_score = score;
            }
          }
          all++;
        }
      }
      if (fill && best)
        best[t] = best_class;
      for (uint64_t e = row_ptr[t]; e < row_ptr[t + 1]; e++)
        count[col[e]] = 0;
    }
    if (!fill) {
      kept_ptr[n_texts] = all;
      *n_kept = all;
      if (counts_only)
        break; /* the call only counts */
      if (all > kept_capacity)
        rc = ACM_GPU_E_OVERFLOW;
    }
  }
  free (count);
  return rc;
}

/* a kept pair of one column: the order of TOP is score descending, text ascending */
typedef struct {
  int64_t score;
  uint32_t text;
} ScoreTopItem;

static int
cmp_score_top (const void *a, const void *b) {
  const ScoreTopItem *x = a, *y = b;
  if (x->score != y->score)
    return x->score > y->score ? -1 : 1;
  return x->text < y->text ? -1 : x->text > y->text;
}

/* TOP of a kept matrix (include/acm_score.h): the kept pairs are put together by class (a counting sort,
 * texts ascending within a class), every column is sorted and its first k entries are taken. */
int
acm_score_top (const uint64_t *kept_ptr, const uint32_t *kept_class, const int64_t *kept_score, uint64_t n_texts, uint64_t n_classes, uint32_t k,
               uint64_t *class_hits, uint32_t *top_n, uint32_t *top_text, int64_t *top_score) {
  if (!kept_ptr || kept_ptr[0] != 0 || n_texts >= (1ull << 31) || n_classes >= (1ull << 31) || k > ACM_SCORE_TOP_MAX ||
      (n_classes && (!class_hits || !top_n || (k && (!top_text || !top_score)))))
    return ACM_GPU_E_ARG;
  for (uint64_t t = 0; t < n_texts; t++)
    if (kept_ptr[t] > kept_ptr[t + 1])
      return ACM_GPU_E_ARG;
  const uint64_t n = kept_ptr[n_texts];
  if (n && (!kept_class || !kept_score))
    return ACM_GPU_E_ARG;
  for (uint64_t e = 0; e < n; e++)
    if (kept_class[e] >= n_classes)
      return ACM_GPU_E_ARG;
  uint64_t *begin = calloc (n_classes + 1, sizeof (uint64_t));
  ScoreTopItem *item = malloc ((n ? n : 1) * sizeof *item);
  if (!begin || !item) {
    free (begin);
    free (item);
    return ACM_GPU_E_NOMEM;
  }
  for (uint64_t e = 0; e < n; e++)
    begin[kept_class[e] + 1]++;
  for (uint64_t c = 0; c < n_classes; c++) {
    class_hits[c] = begin[c + 1];
    begin[c + 1] += begin[c];
  }
  for (uint64_t t = 0; t < n_texts; t++)
    for (uint64_t e = kept_ptr[t]; e < kept_ptr[t + 1]; e++)
      item[begin[kept_class[e]]++] = (ScoreTopItem){ kept_score[e], (uint32_t)t };
  /* (begin[c] has moved on to the end of column c) */
  for (uint64_t c = 0; c < n_classes; c++) {
    const uint64_t hits = class_hits[c];
    ScoreTopItem *column = item + (begin[c] - hits);
    if (k)
      qsort (column, hits, sizeof *column, cmp_score_top);
    top_n[c] = (uint32_t)(hits < k ? hits : k);
    for (uint32_t j = 0; j < k; j++) {
      top_text[c * k + j] = j < top_n[c] ? column[j].text : ACM_SCORE_NONE;
      top_score[c * k + j] = j < top_n[c] ? column[j].score : 0;
    }
  }
  free (item);
  free (begin);
  return ACM_GPU_OK;
}

/* The inverted index of a count matrix in CSR form (include/acm_index.h): the plain sequential
 * transposition.  The lists' lengths are counted into post_ptr[] and summed; the fill walks the rows
 * in order, so every list ascends by text id, with post_ptr[k] as list k's cursor, and moves the
 * pointers back by one place behind it. */
int
acm_index_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts, uint64_t n_keywords, uint64_t text_base,
                  uint64_t *post_ptr, uint32_t *post_text, uint64_t *post_count, uint64_t post_capacity, uint64_t *nnz) {
  if (!row_ptr || row_ptr[0] != 0 || !post_ptr || !nnz || n_texts >= (1ull << 31) || n_keywords >= (1ull << 32) || text_base > (1ull << 32) ||
      text_base + n_texts > (1ull << 32) || post_capacity >= (1ull << 31))
    return ACM_GPU_E_ARG;
  for (uint64_t t = 0; t < n_texts; t++)
    if (row_ptr[t] > row_ptr[t + 1])
      return ACM_GPU_E_ARG;
  const uint64_t all = row_ptr[n_texts];
  if (all && (!col || !val))
    return ACM_GPU_E_ARG;
  for (uint64_t e = 0; e < all; e++)
    if (col[e] >= n_keywords)
      return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k <= n_keywords; k++)
    post_ptr[k] = 0;
  for (uint64_t e = 0; e < all; e++)
    post_ptr[col[e] + 1]++;
  for (uint64_t k = 0; k < n_keywords; k++)
    post_ptr[k + 1] += post_ptr[k];
  *nnz = all;
  if (!post_text || !post_count) /* the call only counts */
    return ACM_GPU_OK;
  if (all > post_capacity)
    return ACM_GPU_E_OVERFLOW;
  for (uint64_t t = 0; t < n_texts; t++)
    for (uint64_t e = row_ptr[t]; e < row_ptr[t + 1]; e++) {
      const uint64_t at = post_ptr[col[e]]++;
      post_text[at] = (uint32_t)(text_base + t);
      post_count[at] = val[e];
    }
  for (uint64_t k = n_keywords; k > 0; k--) /* (post_ptr[k] has moved on to the end of k's list) */
    post_ptr[k] = post_ptr[k - 1];
  post_ptr[0] = 0;
  return ACM_GPU_OK;
}

/* CONCAT of two indexes (include/acm_index.h): per keyword A's list, then B's */
int
acm_index_concat (const uint64_t *a_ptr, const uint32_t *a_text, const uint64_t *a_count, uint64_t n_keywords_a, const uint64_t *b_ptr,
                  const uint32_t *b_text, const uint64_t *b_count, uint64_t n_keywords_b, uint64_t *out_ptr, uint32_t *out_text, uint64_t *out_count,
                  uint64_t out_capacity, uint64_t *out_nnz) {
  if (!a_ptr || a_ptr[0] != 0 || !b_ptr || b_ptr[0] != 0 || !out_ptr || !out_nnz || n_keywords_a > n_keywords_b || n_keywords_b >= (1ull << 32) ||
      out_capacity >= (1ull << 31))
    return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k < n_keywords_a; k++)
    if (a_ptr[k] > a_ptr[k + 1])
      return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k < n_keywords_b; k++)
    if (b_ptr[k] > b_ptr[k + 1])
      return ACM_GPU_E_ARG;
  if ((a_ptr[n_keywords_a] && (!a_text || !a_count)) || (b_ptr[n_keywords_b] && (!b_text || !b_count)))
    return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k < n_keywords_a; k++)
    if (a_ptr[k] < a_ptr[k + 1] && b_ptr[k] < b_ptr[k + 1] && b_text[b_ptr[k]] <= a_text[a_ptr[k + 1] - 1])
      return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k <= n_keywords_b; k++)
    out_ptr[k] = a_ptr[k < n_keywords_a ? k : n_keywords_a] + b_ptr[k];
  const uint64_t all = out_ptr[n_keywords_b];
  *out_nnz = all;
  if (!out_text || !out_count) /* the call only counts */
    return ACM_GPU_OK;
  if (all > out_capacity)
    return ACM_GPU_E_OVERFLOW;
  for (uint64_t k = 0; k < n_keywords_b; k++) {
    uint64_t at = out_ptr[k];
    for (uint64_t e = k < n_keywords_a ? a_ptr[k] : 0, end = k < n_keywords_a ? a_ptr[k + 1] : 0; e < end; e++, at++) {
      out_text[at] = a_text[e];
      out_count[at] = a_count[e];
    }
    for (uint64_t e = b_ptr[k]; e < b_ptr[k + 1]; e++, at++) {
      out_text[at] = b_text[e];
      out_count[at] = b_count[e];
    }
  }
  return ACM_GPU_OK;
}

/* The co-occurrence matrix of a count matrix in CSR form (include/acm_cooccur.h): the plain sequential
 * definition.  Every contributing row is expanded into its pair instances (a << 32 | b, weight), the
 * instances are sorted by key, and every run of equal keys is one entry: its length, or the sum of its
 * weights modulo 2^64.  Memory: 16 bytes per pair instance. */
typedef struct {
  uint64_t key, w;
} CooccurPair;

static int
cooccur_pair_cmp (const void *x, const void *y) {
  const uint64_t a = ((const CooccurPair *)x)->key, b = ((const CooccurPair *)y)->key;
  return a < b ? -1 : a > b;
}

/* a pointer array of n + 1 entries begins with 0 and never decreases; its rows ascend strictly by col, every col below `cols` */
static int
cooccur_csr_ok (const uint64_t *ptr, const uint32_t *col, uint64_t n, uint64_t cols) {
  if (!ptr || ptr[0] != 0)
    return 0;
  for (uint64_t t = 0; t < n; t++)
    if (ptr[t] > ptr[t + 1])
      return 0;
  if (ptr[n] && !col)
    return 0;
  for (uint64_t t = 0; t < n; t++)
    for (uint64_t e = ptr[t]; e < ptr[t + 1]; e++)
      if (col[e] >= cols || (e > ptr[t] && col[e] <= col[e - 1]))
        return 0;
  return 1;
}

int
acm_cooccur_matrix (const uint64_t *row_ptr, const uint32_t *col, const uint64_t *val, uint64_t n_texts, uint64_t n_keywords, uint32_t flags,
                    uint64_t row_limit, uint64_t *co_ptr, uint32_t *co_col, uint64_t *co_val, uint64_t out_capacity, uint64_t *nnz, uint64_t *cross,
                    uint64_t *skipped) {
  if (!co_ptr || !nnz || (flags & ~(ACM_COOCCUR_PRODUCT | ACM_COOCCUR_DIAGONAL)) || n_texts >= (1ull << 31) || n_keywords >= (1ull << 32) ||
      out_capacity >= (1ull << 31) || !cooccur_csr_ok (row_ptr, col, n_texts, n_keywords) || (row_ptr[n_texts] && !val))
    return ACM_GPU_E_ARG;
  const int product = (flags & ACM_COOCCUR_PRODUCT) != 0, diagonal = (flags & ACM_COOCCUR_DIAGONAL) != 0;
  uint64_t n_cross = 0, n_skipped = 0;
  for (uint64_t t = 0; t < n_texts; t++) {
    const uint64_t r = row_ptr[t + 1] - row_ptr[t]; /* (at most n_keywords: the row ascends strictly) */
    if (row_limit && r > row_limit) {
      n_skipped++;
      continue;
    }
    const uint64_t p = r * (r - 1 + 2 * (uint64_t)diagonal) / 2;
    if (n_cross + p < n_cross)
      return ACM_GPU_E_NOMEM;
    n_cross += p;
  }
  if (n_cross > SIZE_MAX / sizeof (CooccurPair))
    return ACM_GPU_E_NOMEM;
  CooccurPair *pair = malloc (n_cross ? n_cross * sizeof *pair : 1);
  if (!pair)
    return ACM_GPU_E_NOMEM;
  uint64_t at = 0;
  for (uint64_t t = 0; t < n_texts; t++) {
    const uint64_t begin = row_ptr[t], end = row_ptr[t + 1];
    if (row_limit && end - begin > row_limit)
      continue;
    for (uint64_t i = begin; i < end; i++)
      for (uint64_t j = diagonal ? i : i + 1; j < end; j++) {
        pair[at].key = ((uint64_t)col[i] << 32) | col[j];
        pair[at++].w = product ? val[i] * val[j] : 1;
      }
  }
  qsort (pair, n_cross, sizeof *pair, cooccur_pair_cmp);
  for (uint64_t k = 0; k <= n_keywords; k++)
    co_ptr[k] = 0;
  uint64_t all = 0;
  for (uint64_t q = 0; q < n_cross; q++)
    if (q == 0 || pair[q].key != pair[q - 1].key) {
      co_ptr[(pair[q].key >> 32) + 1]++;
      all++;
    }
  for (uint64_t k = 0; k < n_keywords; k++)
    co_ptr[k + 1] += co_ptr[k];
  *nnz = all;
  if (cross)
    *cross = n_cross;
  if (skipped)
    *skipped = n_skipped;
  int rc = ACM_GPU_OK;
  if (co_col && co_val) { /* (else the call only counts) */
    if (all > out_capacity)
      rc = ACM_GPU_E_OVERFLOW;
    else
      for (uint64_t q = 0, e = 0; q < n_cross; e++) {
        uint64_t sum = 0;
        const uint64_t key = pair[q].key;
        for (; q < n_cross && pair[q].key == key; q++)
          sum += pair[q].w;
        co_col[e] = (uint32_t)key;
        co_val[e] = sum;
      }
  }
  free (pair);
  return rc;
}

/* ADD of two co-occurrence matrices (include/acm_cooccur.h): a two-pointer merge per row, run twice: to count, then to fill */
int
acm_cooccur_add (const uint64_t *a_ptr, const uint32_t *a_col, const uint64_t *a_val, uint64_t n_keywords_a, const uint64_t *b_ptr, const uint32_t *b_col,
                 const uint64_t *b_val, uint64_t n_keywords_b, uint64_t *out_ptr, uint32_t *out_col, uint64_t *out_val, uint64_t out_capacity,
                 uint64_t *out_nnz) {
  if (!out_ptr || !out_nnz || n_keywords_a > n_keywords_b || n_keywords_b >= (1ull << 32) || out_capacity >= (1ull << 31) ||
      !cooccur_csr_ok (a_ptr, a_col, n_keywords_a, n_keywords_b) || !cooccur_csr_ok (b_ptr, b_col, n_keywords_b, n_keywords_b) ||
      (a_ptr[n_keywords_a] && !a_val) || (b_ptr[n_keywords_b] && !b_val))
    return ACM_GPU_E_ARG;
  for (int fill = 0; fill < 2; fill++) {
    uint64_t at = 0;
    for (uint64_t k = 0; k < n_keywords_b; k++) {
      uint64_t i = k < n_keywords_a ? a_ptr[k] : 0, j = b_ptr[k];
      const uint64_t i_end = k < n_keywords_a ? a_ptr[k + 1] : 0, j_end = b_ptr[k + 1];
      if (!fill)
        out_ptr[k] = at;
      while (i < i_end || j < j_end) {
        const int from_a = i < i_end && (j >= j_end || a_col[i] <= b_col[j]), from_b = j < j_end && (i >= i_end || b_col[j] <= a_col[i]);
        if (fill) {
          out_col[at] = from_a ? a_col[i] : b_col[j];
          out_val[at] = (from_a ? a_val[i] : 0) + (from_b ? b_val[j] : 0);
        }
        i += from_a;
        j += from_b;
        at++;
      }
    }
    if (!fill) {
      out_ptr[n_keywords_b] = at;
      *out_nnz = at;
      if (!out_col || !out_val) /* the call only counts */
        return ACM_GPU_OK;
      if (at > out_capacity)
        return ACM_GPU_E_OVERFLOW;
    }
  }
  return ACM_GPU_OK;
}

/* SELECT of records in canonical order (include/acm_gpu.h), in place in the front of the array: the
 * plain sequential greedy pass.  The order is by end and the rule goes by start, so a round looks
 * at a window: from the first record that ends at or behind p up to the first that ends lmax or
 * more behind the best start so far (lmax = the longest record of the set) -- that one and every
 * later one starts behind it.  Everything up to the record taken ends in front of the new p: the
 * output never overwrites a record that is still to be read.  Starts are signed, so that a record
 * whose length exceeds end_pos + 1 (acm_scan_from's, a flow's) keeps its place in front. */
uint64_t
acm_select_records (ACMRecord *records, uint64_t n) {
  if (!records)
    return 0;
  uint32_t lmax = 0;
  for (uint64_t j = 0; j < n; j++)
    if (records[j].length > lmax)
      lmax = records[j].length;
  uint64_t out = 0, i = 0;
  int64_t p = INT64_MIN;
  while (i < n) {
    uint64_t best = n;
    int64_t bstart = 0;
    for (uint64_t j = i; j < n; j++) {
      const ACMRecord *r = &records[j];
      if (best != n && (int64_t)r->end_pos - bstart >= (int64_t)lmax)
        break;
      const int64_t start = (int64_t)r->end_pos + 1 - (int64_t)r->length;
      if (start < p)
        continue;
      const ACMRecord *b = best != n ? &records[best] : NULL;
      if (!b || start < bstart || (start == bstart && (r->length > b->length || (r->length == b->length && r->keyword_id < b->keyword_id)))) {
        best = j;
        bstart = start;
      }
    }
    if (best == n)
      break;
    const ACMRecord take = records[best];
    records[out++] = take;
    p = (int64_t)take.end_pos + 1;
    while (i < n && (int64_t)records[i].end_pos < p)
      i++;
  }
  return out;
}

/* SEGMENT of records in canonical order (include/acm_segment.h), in place in the front of the array:
 * the definition run sequentially, over the records and not over the positions -- V[i] is best[] behind
 * record i among the records up to i, so V of the last record of an end class is best[end + 1], and
 * best[] at a start is V of the last record that ends in front of it plus the uncovered symbols
 * between.  Everything is checked first, so that nothing is modified when the call fails.  Starts are
 * signed.  The output never overwrites a record that is still to be read: it goes forward and holds
 * fewer records than were read. */
int
acm_segment_records (ACMRecord *records, uint64_t n, const uint32_t *cost, uint64_t n_keywords, uint32_t gap_cost, uint64_t *n_selected,
                     uint64_t sums[2]) {
  const uint32_t limit = 1u << 24;
  if (!n_selected || (n && !records) || (n_keywords && !cost) || gap_cost >= limit || n >= (1ull << 32) - 1)
    return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k < n_keywords; k++)
    if (cost[k] >= limit)
      return ACM_GPU_E_ARG;
  /* every position is taken relative to the first record's end, the smallest: any 64-bit end_pos is
   * taken, bit 63 included, and only the differences have to fit a signed number */
  const uint64_t ref = n ? records[0].end_pos : 0;
#define REL_END(i) ((int64_t)(records[i].end_pos - ref))
  int64_t base = INT64_MAX;
  for (uint64_t i = 0; i < n; i++) {
    const ACMRecord *r = &records[i];
    if (r->keyword_id >= n_keywords || r->length == 0 || (i && r->end_pos < records[i - 1].end_pos) || r->end_pos - ref >= (1ull << 40))
      return ACM_GPU_E_ARG;
    const int64_t start = REL_END (i) + 1 - (int64_t)r->length;
    if (start < base)
      base = start;
  }
  if (n && (uint64_t)(REL_END (n - 1) - base) >= (1ull << 40))
    return ACM_GPU_E_ARG;
  *n_selected = 0;
  if (sums)
    sums[0] = sums[1] = 0;
  if (n == 0)
    return ACM_GPU_OK;
  const uint32_t none = 0xFFFFFFFFu;
  uint64_t *V = malloc (n * sizeof *V);
  uint32_t *prev = malloc (n * sizeof *prev), *choice = malloc (n * sizeof *choice), *cfirst = malloc (n * sizeof *cfirst);
  unsigned char *taken = calloc (n, 1);
  int rc = ACM_GPU_E_NOMEM;
  if (V && prev && choice && cfirst && taken) {
    const uint64_t gap = gap_cost;
    uint64_t gap_path = 0, best_w = 0;
    uint32_t best_i = none, cls = 0;
    for (uint64_t i = 0; i < n; i++) {
      const ACMRecord *r = &records[i];
      const int64_t end = REL_END (i), start = end + 1 - (int64_t)r->length;
      uint64_t lo = 0, hi = i; /* the records in front of lo end in front of start, those from hi on do not */
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (REL_END (mid) < start)
          lo = mid + 1;
        else
          hi = mid;
      }
      prev[i] = lo ? (uint32_t)(lo - 1) : none;
      if (i == 0 || records[i - 1].end_pos != r->end_pos) { /* a new end class */
        gap_path = i ? V[i - 1] + gap * (uint64_t)(end - REL_END (i - 1)) : gap * (uint64_t)(end + 1 - base);
        best_i = none;
        cls = (uint32_t)i;
      }
      const uint64_t w = (lo ? V[lo - 1] + gap * (uint64_t)(start - REL_END (lo - 1) - 1) : gap * (uint64_t)(start - base)) + cost[r->keyword_id];
      const ACMRecord *b = best_i != none ? &records[best_i] : NULL;
      if (!b || w < best_w || (w == best_w && (r->length > b->length || (r->length == b->length && r->keyword_id < b->keyword_id)))) {
        best_w = w;
        best_i = (uint32_t)i;
      }
      const int covered = best_w <= gap_path; /* a keyword wins a tie against uncovered symbols */
      V[i] = covered ? best_w : gap_path;
      choice[i] = covered ? best_i : none;
      cfirst[i] = cls;
    }
    for (uint32_t at = (uint32_t)(n - 1);;) { /* backwards from the last class */
      uint32_t next;
      if (choice[at] != none) {
        taken[choice[at]] = 1;
        next = prev[choice[at]];
      } else
        next = cfirst[at] ? cfirst[at] - 1 : none;
      if (next == none)
        break;
      at = next;
    }
    uint64_t out = 0, sum_cost = 0, sum_len = 0;
    for (uint64_t i = 0; i < n; i++)
      if (taken[i]) {
        sum_cost += cost[records[i].keyword_id];
        sum_len += records[i].length;
        records[out++] = records[i];
      }
    *n_selected = out;
    if (sums) {
      sums[0] = sum_cost;
      sums[1] = sum_len;
    }
    rc = ACM_GPU_OK;
  }
  free (taken), free (cfirst), free (choice), free (prev), free (V);
  return rc;
}
#undef REL_END

/* Whether a record breaks the contract of the passes that take a record set (below): its end lies outside
 * [pos_base, pos_base + n_symbols), its length is 0, or it begins in front of pos_base. */
static inline int
record_breaks_contract (const ACMRecord *r, uint64_t pos_base, uint64_t n_symbols) {
  return r->end_pos < pos_base || r->end_pos - pos_base >= n_symbols || r->length == 0 || (uint64_t)r->length - 1 > r->end_pos - pos_base;
}

/* WORDS of a record set (include/acm_gpu.h): the plain sequential pass, in place in the front of the
 * array.  Symbols are unsigned little-endian integers of sym_bytes bytes.  Everything is checked
 * first, so that nothing is modified when the call fails. */
static uint64_t
words_symbol (const unsigned char *text, uint64_t i, uint32_t sb) {
  uint64_t v = 0;
  for (uint32_t k = 0; k < sb; k++)
    v |= (uint64_t)text[i * sb + k] << (8 * k);
  return v;
}

static int
words_is_word (uint64_t x, const unsigned char *ranges, uint32_t n_ranges, uint32_t sb) {
  for (uint32_t j = 0; j < n_ranges; j++)
    if (x >= words_symbol (ranges, 2 * (uint64_t)j, sb) && x <= words_symbol (ranges, 2 * (uint64_t)j + 1, sb))
      return 1;
  return 0;
}

int
acm_internal_words_args_ok (uint32_t sym_bytes, const void *ranges, uint32_t n_ranges, uint32_t flags) {
  if ((sym_bytes != 1 && sym_bytes != 2 && sym_bytes != 4 && sym_bytes != 8) || !ranges || n_ranges == 0 || n_ranges > ACM_WORDS_MAX_RANGES ||
      flags == 0 || flags > ACM_WORDS_BOTH)
    return 0;
  for (uint32_t j = 0; j < n_ranges; j++)
    if (words_symbol (ranges, 2 * (uint64_t)j, sym_bytes) > words_symbol (ranges, 2 * (uint64_t)j + 1, sym_bytes))
      return 0;
  return 1;
}

int
acm_words_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                   const void *ranges, uint32_t n_ranges, uint32_t flags, ACMRecord *records, uint64_t n, uint64_t *n_kept) {
  if (!n_kept || (n_symbols && !text) || (n && !records) || !acm_internal_words_args_ok (sym_bytes, ranges, n_ranges, flags))
    return ACM_GPU_E_ARG;
  if (offsets) {
    if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
  }
  const unsigned char *t = text;
  uint64_t kept = 0;
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord r = records[j];
    const uint64_t e = r.end_pos - pos_base, s = e + 1 - r.length;
    uint64_t t_lo = 0, t_hi = n_symbols; /* the record's text: [t_lo, t_hi) */
    if (offsets) {                       /* (n_texts > 0: a record lies in [0, n_symbols) = [0, offsets[n_texts])) */
      uint64_t lo = 0, hi = n_texts - 1; /* the largest text with offsets[text] <= s */
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= s)
          lo = mid;
        else
          hi = mid - 1;
      }
      t_lo = offsets[lo];
      t_hi = offsets[lo + 1];
      if (e >= t_hi) /* the match spans a cut: no match of any text */
        continue;
    }
    if ((flags & ACM_WORDS_LEFT) && s > t_lo && words_is_word (words_symbol (t, s - 1, sym_bytes), ranges, n_ranges, sym_bytes))
      continue;
    if ((flags & ACM_WORDS_RIGHT) && e + 1 < t_hi && words_is_word (words_symbol (t, e + 1, sym_bytes), ranges, n_ranges, sym_bytes))
      continue;
    records[kept++] = r;
  }
  *n_kept = kept;
  return ACM_GPU_OK;
}

/* acm_scan_words on the host (include/acm_gpu.h): the caller loop, then the sequential pass over
 * what it found -- what ACM_SCAN_PATH_CPU_LOOP runs.  The arguments are checked before the scan. */
int
acm_internal_cpu_scan_words (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const void *ranges, uint32_t n_ranges,
                             uint32_t flags, ACMRecord *records, uint64_t capacity, uint64_t *n_found) {
  if (!m || !n_found || !acm_internal_words_args_ok (sym_bytes, ranges, n_ranges, flags))
    return ACM_GPU_E_ARG;
  const int rc = acm_internal_cpu_scan (m, text, n_symbols, sym_bytes, records, capacity, n_found);
  if (rc)
    return rc;
  return acm_words_records (text, n_symbols, sym_bytes, 0, NULL, 0, ranges, n_ranges, flags, records, *n_found, n_found);
}

/* CHARS (include/acm_chars.h): byte positions and records in code points or UTF-16 units, the plain sequential
 * definition.  Two prefix counts over the text -- non-continuation bytes and, under UTF16, wide leads -- and every
 * answer is a difference of two of their entries.  Everything is checked first, so that nothing is written when the
 * call fails. */
struct chars_rank {
  uint64_t *starts, *wides; /* [n_symbols + 1]; wides NULL under CODEPOINTS */
};

static int
chars_offsets_ok (const uint64_t *offsets, uint64_t n_texts, uint64_t n_symbols) {
  if (!offsets)
    return 1;
  if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
    return 0;
  for (uint64_t t = 0; t < n_texts; t++)
    if (offsets[t] > offsets[t + 1])
      return 0;
  return 1;
}

static int
chars_rank_make (struct chars_rank *R, const unsigned char *text, uint64_t n_symbols, uint32_t unit) {
  R->starts = malloc ((n_symbols + 1) * sizeof (uint64_t));
  R->wides = unit == ACM_CHARS_UTF16 ? malloc ((n_symbols + 1) * sizeof (uint64_t)) : NULL;
  if (!R->starts || (unit == ACM_CHARS_UTF16 && !R->wides)) {
    free (R->starts), free (R->wides);
    return ACM_GPU_E_NOMEM;
  }
  R->starts[0] = 0;
  if (R->wides)
    R->wides[0] = 0;
  for (uint64_t i = 0; i < n_symbols; i++) {
    R->starts[i + 1] = R->starts[i] + ((text[i] & 0xC0) != 0x80);
    if (R->wides)
      R->wides[i + 1] = R->wides[i] + (text[i] >= 0xF0);
  }
  return ACM_GPU_OK;
}

/* count (a, b), a <= b <= n_symbols */
static uint64_t
chars_count (const struct chars_rank *R, uint64_t a, uint64_t b) {
  return R->starts[b] - R->starts[a] + (R->wides ? R->wides[b] - R->wides[a] : 0);
}

/* the largest text t with offsets[t] <= p (n_texts > 0) */
static uint64_t
chars_text_of (const uint64_t *offsets, uint64_t n_texts, uint64_t p) {
  uint64_t lo = 0, hi = n_texts - 1;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] <= p)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

int
acm_chars_positions (const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, uint32_t unit, const uint64_t *pos, uint64_t n,
                     uint64_t *out) {
  if ((unit != ACM_CHARS_CODEPOINTS && unit != ACM_CHARS_UTF16) || (n_symbols && !text) || (n && (!pos || !out)) ||
      !chars_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  for (uint64_t i = 0; i < n; i++)
    if (pos[i] > n_symbols)
      return ACM_GPU_E_ARG;
  struct chars_rank R;
  const int rc = chars_rank_make (&R, text, n_symbols, unit);
  if (rc)
    return rc;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t lo = offsets && n_texts ? offsets[chars_text_of (offsets, n_texts, pos[i])] : 0;
    out[i] = chars_count (&R, lo, pos[i]);
  }
  free (R.starts), free (R.wides);
  return ACM_GPU_OK;
}

int
acm_chars_records (const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts, uint32_t unit,
                   const ACMRecord *records, uint64_t n, uint64_t *char_start, uint32_t *char_len, uint8_t *edge) {
  if ((unit != ACM_CHARS_CODEPOINTS && unit != ACM_CHARS_UTF16) || (n_symbols && !text) || (n && !records) || (!char_start && !char_len && !edge) ||
      !chars_offsets_ok (offsets, n_texts, n_symbols))
    return ACM_GPU_E_ARG;
  for (uint64_t j = 0; j < n; j++)
    if (record_breaks_contract (&records[j], pos_base, n_symbols))
      return ACM_GPU_E_ARG;
  struct chars_rank R;
  const int rc = chars_rank_make (&R, text, n_symbols, unit);
  if (rc)
    return rc;
  const unsigned char *t = text;
  for (uint64_t j = 0; j < n; j++) {
    const uint64_t e = records[j].end_pos - pos_base, s = e + 1 - records[j].length;
    uint64_t lo = 0, hi = n_symbols; /* the text of s: [lo, hi) */
    if (offsets && n_texts) {
      const uint64_t tx = chars_text_of (offsets, n_texts, s);
      lo = offsets[tx];
      hi = offsets[tx + 1];
    }
    if (char_start)
      char_start[j] = chars_count (&R, lo, s);
    if (char_len)
      char_len[j] = (uint32_t)chars_count (&R, s, e + 1);
    if (edge) /* a boundary: lo, hi, the end of the buffer, or a byte that is no continuation */
      edge[j] = (uint8_t)((s != lo && (t[s] & 0xC0) == 0x80 ? ACM_CHARS_EDGE_START : 0u) |
                          (e + 1 != hi && e + 1 < n_symbols && (t[e + 1] & 0xC0) == 0x80 ? ACM_CHARS_EDGE_END : 0u));
  }
  free (R.starts), free (R.wides);
  return ACM_GPU_OK;
}

/* acm_scan_chars on the host (include/acm_chars.h): the caller loop, then the sequential map of what it found -- what
 * ACM_SCAN_PATH_CPU_LOOP runs.  The text is bytes. */
int
acm_internal_cpu_scan_chars (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint32_t unit, ACMRecord *records,
                             uint64_t *char_start, uint32_t *char_len, uint8_t *edge, uint64_t capacity, uint64_t *n_found) {
  if (!m || !n_found || sym_bytes != 1 || (unit != ACM_CHARS_CODEPOINTS && unit != ACM_CHARS_UTF16) || (!char_start && !char_len && !edge))
    return ACM_GPU_E_ARG;
  const int rc = acm_internal_cpu_scan (m, text, n_symbols, sym_bytes, records, capacity, n_found);
  if (rc)
    return rc;
  return acm_chars_records (text, n_symbols, 0, NULL, 0, unit, records, *n_found, char_start, char_len, edge);
}

/* CONTEXT of a record set (include/acm_gpu.h): the plain sequential pass.  Everything is checked
 * and every window made first.  MERGE walks the records BACKWARDS: over the windowed records hi
 * never decreases, so a record joins the run behind it iff its hi reaches the smallest lo of that
 * run (and, under SYMBOLS, it lies in the same text); a second walk forwards numbers the runs and
 * measures them.  The output is gathered last, when it is known to have room. */
#define CONTEXT_WINDOWLESS 0x80000000u /* in tx[]: the record spans a cut (a text is below 2^31) */

/* the largest text with offsets[text] <= pos, pos in [0, offsets[n_texts]), n_texts > 0 */
static uint64_t
context_text_of (const uint64_t *offsets, uint64_t n_texts, uint64_t pos) {
  uint64_t lo = 0, hi = n_texts - 1;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] <= pos)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

int
acm_context_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                     const ACMRecord *records, uint64_t n, uint32_t before, uint32_t after, uint32_t flags, void *out, uint64_t out_capacity,
                     uint64_t *out_symbols, uint64_t *n_snippets, uint64_t *snip_lo, uint64_t *out_offsets, uint32_t *snip_text, uint32_t *rec_snip,
                     int64_t *rec_at) {
  if (!out_symbols || !n_snippets || (n_symbols && !text) || (n && !records) || n >= (1ull << 31) ||
      (sym_bytes != 1 && sym_bytes != 2 && sym_bytes != 4 && sym_bytes != 8) || flags > (ACM_CONTEXT_TEXTS | ACM_CONTEXT_MERGE) ||
      ((flags & ACM_CONTEXT_TEXTS) && !offsets))
    return ACM_GPU_E_ARG;
  if (offsets) {
    if (n_texts >= (1ull << 31) || offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  const int merge = (flags & ACM_CONTEXT_MERGE) != 0, texts = (flags & ACM_CONTEXT_TEXTS) != 0;
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
    if (merge && j > 0 && records[j - 1].end_pos > r->end_pos)
      return ACM_GPU_E_ARG;
  }
  /* the windows; MERGE: begin[j] says that a snippet begins at record j, lo[j] is then its first symbol */
  uint64_t *lo = malloc ((n ? n : 1) * (2 * sizeof (uint64_t) + sizeof (uint32_t) + 1));
  if (!lo)
    return ACM_GPU_E_NOMEM;
  uint64_t *hi = lo + (n ? n : 1);
  uint32_t *tx = (uint32_t *)(hi + (n ? n : 1));
  unsigned char *begin = (unsigned char *)(tx + (n ? n : 1));
  for (uint64_t j = 0; j < n; j++) {
    const uint64_t e = records[j].end_pos - pos_base, s = e + 1 - records[j].length;
    uint64_t t = 0, t_lo = 0, t_hi = n_symbols; /* the record's text: [t_lo, t_hi) */
    begin[j] = 0;
    if (offsets) { /* (n_texts > 0: a record lies in [0, n_symbols) = [0, offsets[n_texts])) */
      t = context_text_of (offsets, n_texts, s);
      t_lo = offsets[t];
      t_hi = offsets[t + 1];
    }
    tx[j] = (uint32_t)t;
    if (e >= t_hi) { /* the match spans a cut: no match of any text */
      tx[j] |= CONTEXT_WINDOWLESS;
      lo[j] = hi[j] = s;
    } else if (texts) {
      lo[j] = offsets[t > before ? t - before : 0];
      hi[j] = offsets[n_texts - (t + 1) > after ? t + 1 + after : n_texts];
    } else {
      lo[j] = s - t_lo > before ? s - before : t_lo;
      hi[j] = t_hi - (e + 1) > after ? e + 1 + after : t_hi;
    }
  }
  if (merge) {
    uint64_t run_lo = 0, run_first = n; /* the run behind the walk: its smallest lo, its first record (n: none yet) */
    for (uint64_t j = n; j-- > 0;) {
      if (tx[j] & CONTEXT_WINDOWLESS)
        continue;
      if (run_first < n && hi[j] >= run_lo && (texts || tx[j] == tx[run_first])) {
        run_lo = lo[j] < run_lo ? lo[j] : run_lo;
      } else {
        if (run_first < n) {
          begin[run_first] = 1;
          lo[run_first] = run_lo;
        }
        run_lo = lo[j];
      }
      run_first = j;
    }
    if (run_first < n) {
      begin[run_first] = 1;
      lo[run_first] = run_lo;
    }
  }
  /* the snippets: number, place and length; q = the snippet under way (MERGE) */
  uint64_t count = 0, all = 0, q_lo = 0, q_at = 0;
  for (uint64_t j = 0; j < n; j++) {
    const int windowed = !(tx[j] & CONTEXT_WINDOWLESS);
    if (merge ? windowed && begin[j] : 1) {
      q_lo = lo[j];
      q_at = all;
      if (snip_lo)
        snip_lo[count] = q_lo;
      if (out_offsets)
        out_offsets[count] = q_at;
      if (snip_text)
        snip_text[count] = offsets ? (uint32_t)context_text_of (offsets, n_texts, q_lo) : 0;
      count++;
    }
    if (windowed && hi[j] - q_lo > all - q_at) /* (the snippet reaches as far as its records' windows do) */
      all = q_at + (hi[j] - q_lo);
    if (rec_snip)
      rec_snip[j] = windowed ? (uint32_t)(count - 1) : 0xFFFFFFFFu;
    if (rec_at)
      rec_at[j] = windowed ? (int64_t)(q_at + (records[j].end_pos - pos_base + 1 - records[j].length - q_lo)) : -1;
    if (merge && windowed) /* (the snippet's end so far, for the gather) */
      hi[j] = q_lo + (all - q_at);
  }
  if (out_offsets)
    out_offsets[count] = all;
  *n_snippets = count;
  *out_symbols = all;
  int rc = ACM_GPU_OK;
  if (out && all > out_capacity)
    rc = ACM_GPU_E_OVERFLOW;
  else if (out) {
    unsigned char *o = out;
    for (uint64_t j = 0; j < n; j++) {
      const int windowed = !(tx[j] & CONTEXT_WINDOWLESS);
      if (!windowed)
        continue;
      if (!merge) {
        memcpy (o, (const unsigned char *)text + lo[j] * sym_bytes, (hi[j] - lo[j]) * sym_bytes);
        o += (hi[j] - lo[j]) * sym_bytes;
        continue;
      }
      /* the last record of a run holds the run's end: copy when the next windowed record begins one, or there is none */
      uint64_t k = j + 1;
      while (k < n && (tx[k] & CONTEXT_WINDOWLESS))
        k++;
      if (begin[j])
        q_lo = lo[j];
      if (k == n || begin[k]) {
        memcpy (o, (const unsigned char *)text + q_lo * sym_bytes, (hi[j] - q_lo) * sym_bytes);
        o += (hi[j] - q_lo) * sym_bytes;
      }
    }
  }
  free (lo);
  return rc;
}

/* acm_context on the host (include/acm_gpu.h): the caller loop, then the sequential pass over what it
 * found -- what ACM_SCAN_PATH_CPU_LOOP runs.  Without a record array of the caller's the room is the call's own. */
int
acm_internal_cpu_context (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records, uint64_t capacity,
                          uint64_t *n_found, uint32_t before, uint32_t after, uint32_t flags, void *out, uint64_t out_capacity, uint64_t *out_symbols,
                          uint64_t *n_snippets, uint64_t *snip_lo, uint64_t *out_offsets, uint32_t *snip_text, uint32_t *rec_snip, int64_t *rec_at) {
  if (!m || !n_found)
    return ACM_GPU_E_ARG;
  ACMRecord *own = NULL;
  if (!records && capacity) {
    records = own = malloc (capacity * sizeof (ACMRecord));
    if (!own)
      return ACM_GPU_E_NOMEM;
  }
  int rc = acm_internal_cpu_scan (m, text, n_symbols, sym_bytes, records, capacity, n_found);
  if (!rc)
    rc = acm_context_records (text, n_symbols, sym_bytes, 0, NULL, 0, records, *n_found, before, after, flags, out, out_capacity, out_symbols,
                              n_snippets, snip_lo, out_offsets, snip_text, rec_snip, rec_at);
  free (own);
  return rc;
}

/* REPLACE of a text under a selection (include/acm_gpu.h): the plain sequential pass.  The records
 * are checked and the output measured first, so that nothing is written when it has no room. */
int
acm_replace_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base, const ACMRecord *records, uint64_t n,
                     const void *repl_data, const uint64_t *repl_off, uint64_t n_keywords, void *out, uint64_t out_capacity,
                     uint64_t *out_symbols) {
  if (!out_symbols || !sym_bytes || (n_symbols && !text) || (n && !records) || (out_capacity && !out) || (!repl_off && !repl_data))
    return ACM_GPU_E_ARG;
  uint64_t next = 0, need = n_symbols; /* the first symbol no record has taken yet (relative to the text) */
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
    const uint64_t start = r->end_pos - pos_base + 1 - r->length;
    if (start < next)
      return ACM_GPU_E_ARG;
    next = start + r->length;
    if (repl_off) {
      if (r->keyword_id >= n_keywords || repl_off[r->keyword_id] > repl_off[(uint64_t)r->keyword_id + 1] ||
          (repl_off[(uint64_t)r->keyword_id + 1] && !repl_data))
        return ACM_GPU_E_ARG;
      need = need - r->length + (repl_off[(uint64_t)r->keyword_id + 1] - repl_off[r->keyword_id]);
    }
  }
  *out_symbols = need;
  if (need > out_capacity)
    return ACM_GPU_E_OVERFLOW;
  const unsigned char *t = text, *rd = repl_data;
  unsigned char *o = out;
  const size_t sb = sym_bytes;
  uint64_t at = 0; /* symbols of the output so far */
  next = 0;
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    const uint64_t start = r->end_pos - pos_base + 1 - r->length;
    if (start > next)
      memcpy (o + at * sb, t + next * sb, (start - next) * sb);
    at += start - next;
    if (repl_off) {
      const uint64_t rb = repl_off[r->keyword_id], rl = repl_off[(uint64_t)r->keyword_id + 1] - rb;
      if (rl)
        memcpy (o + at * sb, rd + rb * sb, rl * sb);
      at += rl;
    } else {
      for (uint64_t k = 0; k < r->length; k++)
        memcpy (o + (at + k) * sb, rd, sb);
      at += r->length;
    }
    next = start + r->length;
  }
  if (n_symbols > next)
    memcpy (o + at * sb, t + next * sb, (n_symbols - next) * sb);
  return ACM_GPU_OK;
}

/* TOKENS of a text under a selection (include/acm_gpu.h): the plain sequential pass.  One walk does
 * both jobs: with `write` it fills the three token arrays, without it only counts; tok_first[] is
 * written either way.  The caller has checked the records and the offsets. */
static uint64_t
tokens_walk (const unsigned char *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base, const ACMRecord *records, uint64_t n,
             const uint64_t *offsets, uint64_t n_texts, const uint32_t *tok_of, uint32_t gap_base, uint32_t mode, int write, uint32_t *tok_id,
             uint64_t *tok_start, uint32_t *tok_len, uint64_t *tok_first) {
  uint64_t count = 0, next = 0;
  uint64_t t = 0; /* the first text whose tok_first is still to come */
  uint64_t u = 0; /* the first offset behind the gap symbol in hand (RUN) */
  for (uint64_t j = 0; j <= n; j++) {
    const uint64_t start = j < n ? records[j].end_pos - pos_base + 1 - records[j].length : n_symbols;
    uint64_t i = next; /* the gap [next, start) */
    while (i < start && mode != ACM_TOKENS_GAP_DROP) {
      uint64_t end = i + 1;
      if (mode == ACM_TOKENS_GAP_RUN) {
        end = start;
        if (offsets) {
          while (u <= n_texts && offsets[u] <= i)
            u++;
          if (u <= n_texts && offsets[u] < end)
            end = offsets[u];
        }
      }
      while (tok_first && t <= n_texts && offsets[t] <= i)
        tok_first[t++] = count;
      if (write) {
        uint32_t id = gap_base;
        if (mode == ACM_TOKENS_GAP_SYMBOL)
          id += sym_bytes == 1 ? text[i] : (uint32_t)text[2 * i] | ((uint32_t)text[2 * i + 1] << 8);
        tok_id[count] = id;
        if (tok_start)
          tok_start[count] = i + pos_base;
        if (tok_len)
          tok_len[count] = end - i > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(end - i);
      }
      count++;
      i = end;
    }
    if (j == n)
      break;
    while (tok_first && t <= n_texts && offsets[t] <= start)
      tok_first[t++] = count;
    if (write) {
      tok_id[count] = tok_of ? tok_of[records[j].keyword_id] : records[j].keyword_id;
      if (tok_start)
        tok_start[count] = start + pos_base;
      if (tok_len)
        tok_len[count] = records[j].length;
    }
    count++;
    next = start + records[j].length;
  }
  while (tok_first && t <= n_texts)
    tok_first[t++] = count;
  return count;
}

int
acm_tokens_records (const void *text, uint64_t n_symbols, uint32_t sym_bytes, uint64_t pos_base, const ACMRecord *records, uint64_t n,
                    const uint64_t *offsets, uint64_t n_texts, const uint32_t *tok_of, uint64_t n_keywords, uint32_t gap_base, uint32_t mode,
                    uint32_t *tok_id, uint64_t *tok_start, uint32_t *tok_len, uint64_t token_capacity, uint64_t *n_tokens, uint64_t *tok_first) {
  if (!n_tokens || !sym_bytes || (n && !records) || mode > ACM_TOKENS_GAP_DROP || (!offsets && tok_first) || (offsets && n_texts >= (1ull << 31)))
    return ACM_GPU_E_ARG;
  if (mode == ACM_TOKENS_GAP_SYMBOL) {
    if (sym_bytes > 2 || (uint64_t)gap_base > (1ull << 32) - (1ull << (8 * sym_bytes)) || (n_symbols && !text))
      return ACM_GPU_E_ARG;
  }
  if (offsets) {
    if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  uint64_t next = 0, u = 0; /* the first symbol no record has taken yet; the first offset behind the record's start */
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
    const uint64_t start = r->end_pos - pos_base + 1 - r->length;
    if (start < next)
      return ACM_GPU_E_ARG;
    next = start + r->length;
    if (tok_of && r->keyword_id >= n_keywords)
      return ACM_GPU_E_ARG;
    if (offsets) { /* a record lies inside one text */
      while (u <= n_texts && offsets[u] <= start)
        u++;
      if (u <= n_texts && offsets[u] < next)
        return ACM_GPU_E_ARG;
    }
  }
  const unsigned char *t = text;
  *n_tokens = tokens_walk (t, n_symbols, sym_bytes, pos_base, records, n, offsets, n_texts, tok_of, gap_base, mode, 0, NULL, NULL, NULL, tok_first);
  if (!tok_id)
    return ACM_GPU_OK;
  if (*n_tokens > token_capacity)
    return ACM_GPU_E_OVERFLOW;
  (void)tokens_walk (t, n_symbols, sym_bytes, pos_base, records, n, offsets, n_texts, tok_of, gap_base, mode, 1, tok_id, tok_start, tok_len, NULL);
  return ACM_GPU_OK;
}

/* ---- what ACM_SCAN_PATH_CPU_LOOP runs for the other calls of include/acm_gpu.h; arguments as the public call's, behind its checks.
 * The caller loop over one text (offsets NULL) or from the root at every offset of a batch (first[] as acm_internal_cpu_scan_batch's,
 * may be NULL), into a record room the call grows itself: one record per 64 symbols, 1024 at the least, and once more with the
 * number the first scan found.  *records is the caller's to free, whatever is returned. */
static int
cpu_scan_grown (ACMachine *m, const void *text, uint64_t n_symbols, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint64_t *first,
                ACMRecord **records, uint64_t *n_found) {
  uint64_t room = n_symbols / 64 > 1024 ? n_symbols / 64 : 1024;
  *records = NULL;
  for (int attempt = 0; attempt < 2; attempt++) {
    free (*records);
    *records = malloc (room * sizeof (ACMRecord));
    if (!*records)
      return ACM_GPU_E_NOMEM;
    const int rc = offsets ? acm_internal_cpu_scan_batch (m, text, offsets, n_texts, sym_bytes, *records, NULL, first, room, n_found)
                           : acm_internal_cpu_scan (m, text, n_symbols, sym_bytes, *records, room, n_found);
    if (rc != ACM_GPU_E_OVERFLOW)
      return rc;
    room = *n_found;
  }
  return ACM_GPU_E_INTERNAL; /* (keywords inserted between the two scans) */
}

int
acm_internal_cpu_select (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, ACMRecord *records, uint64_t capacity,
                         uint64_t *n_found) {
  const int rc = acm_internal_cpu_scan (m, text, n_symbols, sym_bytes, records, capacity, n_found);
  if (!rc)
    *n_found = acm_select_records (records, *n_found);
  return rc;
}

/* the loop, then SEGMENT.  The table covers every keyword of the machine, as on the GPU paths. */
int
acm_internal_cpu_segment (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint32_t *cost, uint64_t n_keywords,
                          uint32_t gap_cost, ACMRecord *records, uint64_t capacity, uint64_t *n_found, uint64_t sums[2]) {
  if (!m || n_keywords < acm_nb_keywords (m))
    return ACM_GPU_E_ARG;
  for (uint64_t k = 0; k < n_keywords; k++)
    if (cost[k] >= (1u << 24))
      return ACM_GPU_E_ARG;
  int rc = acm_internal_cpu_scan (m, text, n_symbols, sym_bytes, records, capacity, n_found);
  if (!rc)
    rc = acm_segment_records (records, *n_found, cost, n_keywords, gap_cost, n_found, sums);
  return rc;
}

/* the loop, the selection, the sequential pass.  The table covers every keyword of the machine, as on the GPU paths. */
int
acm_internal_cpu_replace (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const void *repl_data, const uint64_t *repl_off,
                          uint64_t n_keywords, void *out, uint64_t out_capacity, uint64_t *out_symbols, uint64_t *n_replaced) {
  if (!m || (repl_off && n_keywords < acm_nb_keywords (m)))
    return ACM_GPU_E_ARG;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, NULL, 0, sym_bytes, NULL, &records, &found);
  if (!rc) {
    found = acm_select_records (records, found);
    if (n_replaced)
      *n_replaced = found;
    rc = acm_replace_records (text, n_symbols, sym_bytes, 0, records, found, repl_data, repl_off, n_keywords, out, out_capacity, out_symbols);
  }
  free (records);
  return rc;
}

/* the same with the token pass (a batch's records never cross a text: one selection serves all texts) */
int
acm_internal_cpu_tokenize (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                           const uint32_t *tok_of, uint64_t n_keywords, uint32_t gap_base, uint32_t mode, uint32_t *tok_id, uint64_t *tok_start,
                           uint32_t *tok_len, uint64_t token_capacity, uint64_t *n_tokens, uint64_t *tok_first, uint64_t *n_selected) {
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, offsets, n_texts, sym_bytes, NULL, &records, &found);
  if (!rc) {
    found = acm_select_records (records, found);
    if (n_selected)
      *n_selected = found;
    rc = acm_tokens_records (text, n_symbols, sym_bytes, 0, records, found, offsets, n_texts, tok_of, n_keywords, gap_base, mode, tok_id, tok_start,
                             tok_len, token_capacity, n_tokens, tok_first);
  }
  free (records);
  return rc;
}

/* the loop, counting per text (into the caller's hits[] or the call's own), then the sequential gather */
int
acm_internal_cpu_grep (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint32_t flags, uint64_t *hits,
                       uint32_t *kept, uint64_t *n_kept, uint64_t *total, void *out, uint64_t out_capacity, uint64_t *out_offsets,
                       uint64_t *out_symbols) {
  uint64_t *own = hits ? NULL : malloc ((n_texts + 1) * sizeof (uint64_t));
  uint64_t *h = hits ? hits : own;
  if (!h)
    return ACM_GPU_E_NOMEM;
  int rc = acm_internal_cpu_grep_hits (m, text, offsets, n_texts, sym_bytes, h);
  if (!rc) {
    if (total) {
      *total = 0;
      for (uint64_t t = 0; t < n_texts; t++)
        *total += h[t];
    }
    rc = acm_grep_gather (text, sym_bytes, offsets, n_texts, h, flags, kept, n_kept, out, out ? out_capacity : 0, out_offsets, out_symbols);
  }
  free (own);
  return rc;
}

/* the loop with first[], then the sequential pass over the records */
int
acm_internal_cpu_tally_batch (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint64_t *row_ptr,
                              uint32_t *col, uint64_t *val, uint64_t nnz_capacity, uint64_t *nnz, uint64_t *total) {
  if (!m || !offsets)
    return ACM_GPU_E_ARG;
  uint64_t *first = malloc ((n_texts + 1) * sizeof (uint64_t));
  if (!first)
    return ACM_GPU_E_NOMEM;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, offsets[n_texts], offsets, n_texts, sym_bytes, first, &records, &found);
  if (!rc) {
    if (total)
      *total = found;
    rc = acm_tally_batch_records (records, first, n_texts, acm_nb_keywords (m), row_ptr, col, val, nnz_capacity, nnz);
  }
  free (records);
  free (first);
  return rc;
}

/* the loop and the count matrix as above, into a room of the call's own that is grown to what the matrix needs;
 * the caller frees the three arrays, whatever comes back */
static int
cpu_tally_batch_grown (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint64_t **row_ptr_out,
                       uint32_t **col_out, uint64_t **val_out, uint64_t *total) {
  uint64_t *row_ptr = malloc ((n_texts + 1) * sizeof (uint64_t));
  uint32_t *col = NULL;
  uint64_t *val = NULL, room = 1024, nnz = 0;
  int rc = row_ptr ? ACM_GPU_OK : ACM_GPU_E_NOMEM;
  for (int attempt = 0; !rc && attempt < 2; attempt++) {
    col = malloc (room * sizeof (uint32_t));
    val = malloc (room * sizeof (uint64_t));
    rc = col && val ? acm_internal_cpu_tally_batch (m, text, offsets, n_texts, sym_bytes, row_ptr, col, val, room, &nnz, total) : ACM_GPU_E_NOMEM;
    if (rc != ACM_GPU_E_OVERFLOW || attempt)
      break;
    free (col);
    free (val);
    col = NULL;
    val = NULL;
    room = nnz;
    rc = ACM_GPU_OK;
  }
  if (rc == ACM_GPU_E_OVERFLOW) /* (the second room is what the first attempt asked for: never expected) */
    rc = ACM_GPU_E_INTERNAL;
  *row_ptr_out = row_ptr;
  *col_out = col;
  *val_out = val;
  return rc;
}

/* that count matrix, then the sequential evaluation */
int
acm_internal_cpu_rules (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, const ACMRuleTerm *terms,
                        const uint64_t *rule_ptr, const uint32_t *need, uint64_t n_rules, uint64_t *fired_ptr, uint32_t *fired, uint64_t fired_capacity,
                        uint64_t *n_fired, uint64_t *total) {
  if (!m || !offsets || !fired_ptr || !n_fired)
    return ACM_GPU_E_ARG;
  const uint64_t n_keywords = acm_nb_keywords (m);
  if (acm_rules_check (terms, rule_ptr, need, n_rules, n_keywords))
    return ACM_GPU_E_ARG;
  uint64_t *row_ptr, *val;
  uint32_t *col;
  int rc = cpu_tally_batch_grown (m, text, offsets, n_texts, sym_bytes, &row_ptr, &col, &val, total);
  if (!rc)
    rc = acm_rules_matrix (row_ptr, col, val, n_texts, n_keywords, terms, rule_ptr, need, n_rules, fired_ptr, fired, fired_capacity, n_fired);
  free (val);
  free (col);
  free (row_ptr);
  return rc;
}

/* the same in front of the scores and, when the kept entries were written and k > 0, their TOP */
int
acm_internal_cpu_score (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, const ACMScoreTerm *terms,
                        const uint64_t *class_ptr, const int64_t *bias, const int64_t *threshold, uint64_t n_classes, uint64_t *kept_ptr,
                        uint32_t *kept_class, int64_t *kept_score, uint64_t kept_capacity, uint64_t *n_kept, uint32_t *best, uint32_t k,
                        uint64_t *class_hits, uint32_t *top_n, uint32_t *top_text, int64_t *top_score, uint64_t *total) {
  if (!m || !offsets || !kept_ptr || !n_kept || k > ACM_SCORE_TOP_MAX)
    return ACM_GPU_E_ARG;
  const uint64_t n_keywords = acm_nb_keywords (m);
  if (acm_score_check (terms, class_ptr, bias, threshold, n_classes, n_keywords))
    return ACM_GPU_E_ARG;
  uint64_t *row_ptr, *val;
  uint32_t *col;
  int rc = cpu_tally_batch_grown (m, text, offsets, n_texts, sym_bytes, &row_ptr, &col, &val, total);
  if (!rc)
    rc = acm_score_matrix (row_ptr, col, val, n_texts, n_keywords, terms, class_ptr, bias, threshold, n_classes, kept_ptr, kept_class, kept_score,
                           kept_capacity, n_kept, best);
  if (!rc && k && kept_class && kept_score && class_hits && top_n && top_text && top_score)
    rc = acm_score_top (kept_ptr, kept_class, kept_score, n_texts, n_classes, k, class_hits, top_n, top_text, top_score);
  free (val);
  free (col);
  free (row_ptr);
  return rc;
}

/* ANCHORED of a batch's records (include/acm_gpu.h): the plain sequential pass, in place in the front
 * of the array.  Everything is checked first, so that nothing is modified when the call fails. */
static uint64_t
anchored_text_of (const uint64_t *offsets, uint64_t n_texts, uint64_t s) {
  uint64_t lo = 0, hi = n_texts - 1; /* the largest text with offsets[text] <= s */
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] <= s)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

int
acm_anchored_records (const uint64_t *offsets, uint64_t n_texts, uint32_t mode, ACMRecord *records, uint64_t n, uint32_t *text_id, uint64_t *first,
                      uint64_t *n_kept) {
  if (!offsets || !n_kept || (n && !records) || mode < ACM_ANCHORED_PREFIXES || mode > ACM_ANCHORED_WHOLE || n_texts >= (1ull << 32) ||
      offsets[0] != 0)
    return ACM_GPU_E_ARG;
  for (uint64_t t = 0; t < n_texts; t++)
    if (offsets[t] > offsets[t + 1])
      return ACM_GPU_E_ARG;
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, 0, offsets[n_texts])) /* (positions from 0; the last offset is the number of symbols) */
      return ACM_GPU_E_ARG;
    if (r->end_pos >= offsets[anchored_text_of (offsets, n_texts, r->end_pos + 1 - r->length) + 1]) /* across a cut */
      return ACM_GPU_E_ARG;
  }
  uint64_t kept = 0, next = 0, last = UINT64_MAX; /* next: the first text whose first[] is still to be set; last: the text of records[kept - 1] */
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord r = records[j];
    const uint64_t s = r.end_pos + 1 - r.length, t = anchored_text_of (offsets, n_texts, s);
    if (s != offsets[t] || (mode == ACM_ANCHORED_WHOLE && r.length != offsets[t + 1] - offsets[t]))
      continue;
    if (mode == ACM_ANCHORED_LONGEST && kept && last == t) { /* a longer prefix of the same text takes the place of the shorter */
      records[kept - 1] = r;
      continue;
    }
    for (; first && next <= t; next++)
      first[next] = kept;
    if (text_id)
      text_id[kept] = (uint32_t)t;
    records[kept++] = r;
    last = t;
  }
  for (; first && next <= n_texts; next++)
    first[next] = kept;
  *n_kept = kept;
  return ACM_GPU_OK;
}

/* acm_scan_anchored on the host (include/acm_gpu.h): the caller loop from the root at every offset into a room of the
 * call's own, then the sequential pass over what it found -- what ACM_SCAN_PATH_CPU_LOOP runs.  offsets[] has been
 * checked by the caller.  records and text_id are written only when the kept records fit; first[] always is. */
int
acm_internal_cpu_scan_anchored (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint32_t mode,
                                ACMRecord *records, uint32_t *text_id, uint64_t *first, uint64_t capacity, uint64_t *n_found) {
  if (!m || !offsets || !n_found || (capacity && !records) || mode < ACM_ANCHORED_PREFIXES || mode > ACM_ANCHORED_WHOLE)
    return ACM_GPU_E_ARG;
  ACMRecord *found_rec;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, offsets[n_texts], offsets, n_texts, sym_bytes, NULL, &found_rec, &found);
  uint32_t *tid = !rc && text_id ? malloc ((found + 1) * sizeof (uint32_t)) : NULL;
  if (!rc && text_id && !tid)
    rc = ACM_GPU_E_NOMEM;
  if (!rc)
    rc = acm_anchored_records (offsets, n_texts, mode, found_rec, found, tid, first, n_found);
  if (!rc && *n_found > capacity)
    rc = ACM_GPU_E_OVERFLOW;
  if (!rc && *n_found) {
    memcpy (records, found_rec, *n_found * sizeof (ACMRecord));
    if (text_id)
      memcpy (text_id, tid, *n_found * sizeof (uint32_t));
  }
  free (tid);
  free (found_rec);
  return rc;
}

/* acm_lookup on the host: the same loop, PREFIXES in place, then LONGEST of it and WHOLE of a copy of it */
int
acm_internal_cpu_lookup (ACMachine *m, const void *text, const uint64_t *offsets, uint64_t n_texts, uint32_t sym_bytes, uint32_t *whole_id,
                         uint32_t *prefix_id, uint32_t *prefix_len) {
  if (!m || !offsets || (!whole_id && !prefix_id && !prefix_len))
    return ACM_GPU_E_ARG;
  ACMRecord *rec, *copy = NULL;
  uint32_t *tid = NULL;
  uint64_t found = 0, n_longest = 0, n_whole = 0;
  int rc = cpu_scan_grown (m, text, offsets[n_texts], offsets, n_texts, sym_bytes, NULL, &rec, &found);
  if (!rc)
    rc = acm_anchored_records (offsets, n_texts, ACM_ANCHORED_PREFIXES, rec, found, NULL, NULL, &found);
  if (!rc) {
    copy = malloc ((found + 1) * sizeof (ACMRecord));
    tid = malloc ((found + 1) * sizeof (uint32_t));
    rc = copy && tid ? ACM_GPU_OK : ACM_GPU_E_NOMEM;
  }
  if (!rc) {
    memcpy (copy, rec, found * sizeof (ACMRecord));
    for (uint64_t t = 0; t < n_texts; t++) {
      if (whole_id)
        whole_id[t] = ACM_LOOKUP_NONE;
      if (prefix_id)
        prefix_id[t] = ACM_LOOKUP_NONE;
      if (prefix_len)
        prefix_len[t] = 0;
    }
    rc = acm_anchored_records (offsets, n_texts, ACM_ANCHORED_LONGEST, rec, found, tid, NULL, &n_longest);
  }
  for (uint64_t j = 0; !rc && j < n_longest; j++) {
    if (prefix_id)
      prefix_id[tid[j]] = rec[j].keyword_id;
    if (prefix_len)
      prefix_len[tid[j]] = rec[j].length;
  }
  if (!rc)
    rc = acm_anchored_records (offsets, n_texts, ACM_ANCHORED_WHOLE, copy, found, tid, NULL, &n_whole);
  for (uint64_t j = 0; !rc && whole_id && j < n_whole; j++)
    whole_id[tid[j]] = copy[j].keyword_id;
  free (tid);
  free (copy);
  free (rec);
  return rc;
}

/* ---- keyword patterns with don't-care gaps (include/acm_gpu.h): the argument checks, the plain sequential PATTERNS of a record
 * set in canonical order, and acm_scan_patterns' host path. */
int
acm_patterns_check (const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, uint64_t n_keywords) {
  if (!pat_ptr || pat_ptr[0] != 0 || n_patterns >= (1ull << 31))
    return ACM_GPU_E_ARG;
  for (uint64_t p = 0; p < n_patterns; p++)
    if (pat_ptr[p] >= pat_ptr[p + 1]) /* decreasing, or a pattern without terms */
      return ACM_GPU_E_ARG;
  if (pat_ptr[n_patterns] >= (1ull << 31) || (n_patterns && !terms))
    return ACM_GPU_E_ARG;
  for (uint64_t i = 0; i < pat_ptr[n_patterns]; i++)
    if (terms[i].length == 0 || (uint64_t)terms[i].offset + terms[i].length >= (1ull << 31) || terms[i].keyword_id >= n_keywords)
      return ACM_GPU_E_ARG;
  return ACM_GPU_OK;
}

/* a pattern under its anchor -- the term with the greatest offset + length, the lowest index among equals: its match ends where
 * the pattern's does */
struct pat_post {
  uint32_t keyword_id, length; /* the anchor term's */
  uint32_t L, pattern;
};

/* by anchor keyword, then L descending, then pattern id ascending: the order of a keyword's postings */
static int
pat_post_cmp (const void *a, const void *b) {
  const struct pat_post *x = a, *y = b;
  if (x->keyword_id != y->keyword_id)
    return x->keyword_id < y->keyword_id ? -1 : 1;
  if (x->L != y->L)
    return x->L > y->L ? -1 : 1;
  return x->pattern < y->pattern ? -1 : x->pattern > y->pattern;
}

/* the output order inside a group of equal end_pos: length descending, then pattern id ascending */
static int
pat_out_cmp (const void *a, const void *b) {
  const ACMRecord *x = a, *y = b;
  if (x->length != y->length)
    return x->length > y->length ? -1 : 1;
  return x->keyword_id < y->keyword_id ? -1 : x->keyword_id > y->keyword_id;
}

/* whether the record (end_pos, length, keyword_id) is in records[0 .. n), which are in canonical order (end_pos ascending, length
 * descending: the pair is unique) */
static int
pat_has_record (const ACMRecord *records, uint64_t n, uint64_t end_pos, uint32_t length, uint32_t keyword_id) {
  uint64_t lo = 0, hi = n; /* the first record at or behind the key */
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (records[mid].end_pos < end_pos || (records[mid].end_pos == end_pos && records[mid].length > length))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && records[lo].end_pos == end_pos && records[lo].length == length && records[lo].keyword_id == keyword_id;
}

/* whether the pattern of posting q matches with its anchor at record r (its keyword is the posting's) */
static int
pat_matches (const ACMRecord *records, uint64_t n, const ACMRecord *r, const struct pat_post *q, uint64_t n_symbols, uint64_t pos_base,
             const uint64_t *offsets, uint64_t n_texts, const ACMPatternTerm *terms, const uint64_t *pat_ptr) {
  const uint64_t e = r->end_pos - pos_base;
  if (r->length != q->length || (uint64_t)q->L - 1 > e)
    return 0;
  const uint64_t S = e + 1 - q->L;
  uint64_t t_hi = n_symbols; /* where the text of S ends */
  if (offsets) {
    uint64_t lo = 0, hi = n_texts - 1; /* the largest text with offsets[text] <= S (S < n_symbols: there are texts) */
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (offsets[mid] <= S)
        lo = mid;
      else
        hi = mid - 1;
    }
    t_hi = offsets[lo + 1];
  }
  if (e >= t_hi)
    return 0;
  for (uint64_t i = pat_ptr[q->pattern]; i < pat_ptr[q->pattern + 1]; i++) {
    const ACMPatternTerm *term = &terms[i];
    if (!pat_has_record (records, n, pos_base + S + term->offset + term->length - 1, term->length, term->keyword_id))
      return 0;
  }
  return 1;
}

int
acm_patterns_records (const ACMRecord *records, uint64_t n, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                      const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, uint64_t n_keywords, ACMRecord *out,
                      uint64_t out_capacity, uint64_t *n_found) {
  if (!n_found || (n && !records) || (out_capacity && !out) || acm_patterns_check (terms, pat_ptr, n_patterns, n_keywords))
    return ACM_GPU_E_ARG;
  if (offsets) {
    if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
  }
  struct pat_post *post = malloc ((n_patterns ? n_patterns : 1) * sizeof *post);
  if (!post)
    return ACM_GPU_E_NOMEM;
  for (uint64_t p = 0; p < n_patterns; p++) {
    uint64_t anchor = pat_ptr[p];
    for (uint64_t i = pat_ptr[p] + 1; i < pat_ptr[p + 1]; i++)
      if (terms[i].offset + terms[i].length > terms[anchor].offset + terms[anchor].length)
        anchor = i;
    post[p] = (struct pat_post){ terms[anchor].keyword_id, terms[anchor].length, terms[anchor].offset + terms[anchor].length, (uint32_t)p };
  }
  qsort (post, n_patterns, sizeof *post, pat_post_cmp);
  /* two passes over the records as anchors: the count, then -- when the matches fit -- the matches themselves */
  uint64_t found = 0;
  for (int fill = 0; fill < 2; fill++) {
    found = 0;
    for (uint64_t j = 0; j < n; j++) {
      const ACMRecord *r = &records[j];
      uint64_t lo = 0, hi = n_patterns; /* the keyword's first posting */
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (post[mid].keyword_id < r->keyword_id)
          lo = mid + 1;
        else
          hi = mid;
      }
      for (uint64_t q = lo; q < n_patterns && post[q].keyword_id == r->keyword_id; q++)
        if (pat_matches (records, n, r, &post[q], n_symbols, pos_base, offsets, n_texts, terms, pat_ptr)) {
          if (fill)
            out[found] = (ACMRecord){ r->end_pos, post[q].L, post[q].pattern };
          found++;
        }
    }
    if (!out || found > out_capacity) /* the call only counts, or the matches have no room */
      break;
  }
  free (post);
  *n_found = found;
  if (!out)
    return ACM_GPU_OK;
  if (found > out_capacity)
    return ACM_GPU_E_OVERFLOW;
  /* matches of one end can come from several anchor records and interleave in L then */
  for (uint64_t b = 0; b < found;) {
    uint64_t e = b + 1;
    while (e < found && out[e].end_pos == out[b].end_pos)
      e++;
    if (e - b > 1)
      qsort (out + b, e - b, sizeof *out, pat_out_cmp);
    b = e;
  }
  return ACM_GPU_OK;
}

/* the checks acm_scan_patterns makes on every path: acm_patterns_check against the machine's keywords, and every term's
 * length is its keyword's */
int
acm_internal_patterns_machine_check (ACMachine *m, const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns) {
  if (!m)
    return ACM_GPU_E_ARG;
  int rc = ACM_GPU_OK;
  acm_internal_lock (m);
  rc = acm_patterns_check (terms, pat_ptr, n_patterns, m->nb_keywords);
  for (uint64_t i = 0; !rc && i < pat_ptr[n_patterns]; i++)
    if (m->keywords[terms[i].keyword_id]->depth != terms[i].length)
      rc = ACM_GPU_E_ARG;
  acm_internal_unlock (m);
  return rc;
}

/* acm_scan_patterns on the host: the caller loop (from the root at every offset of a batch), then the sequential pass over
 * what it found -- what ACM_SCAN_PATH_CPU_LOOP runs.  The public call has checked the arguments. */
int
acm_internal_cpu_scan_patterns (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                const ACMPatternTerm *terms, const uint64_t *pat_ptr, uint64_t n_patterns, ACMRecord *out, uint64_t out_capacity,
                                uint64_t *n_found) {
  if (!m || !n_found)
    return ACM_GPU_E_ARG;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, offsets, n_texts, sym_bytes, NULL, &records, &found);
  if (!rc)
    rc = acm_patterns_records (records, found, n_symbols, 0, offsets, n_texts, terms, pat_ptr, n_patterns, acm_nb_keywords (m), out, out_capacity,
                               n_found);
  free (records);
  return rc;
}

/* ---- keyword chains with bounded gaps (include/acm_gpu.h): the argument checks, the plain sequential CHAINS of a record set in
 * canonical order, and acm_scan_chains' host path. */
int
acm_chains_check (const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, uint64_t n_keywords) {
  if (!chain_ptr || chain_ptr[0] != 0 || n_chains >= (1ull << 31))
    return ACM_GPU_E_ARG;
  for (uint64_t c = 0; c < n_chains; c++)
    if (chain_ptr[c] >= chain_ptr[c + 1] || chain_ptr[c + 1] - chain_ptr[c] > ACM_CHAIN_TERMS_MAX) /* decreasing, no term, too many */
      return ACM_GPU_E_ARG;
  if (chain_ptr[n_chains] >= (1ull << 31) || (n_chains && !terms))
    return ACM_GPU_E_ARG;
  for (uint64_t c = 0; c < n_chains; c++)
    for (uint64_t i = chain_ptr[c]; i < chain_ptr[c + 1]; i++) {
      if (terms[i].gap_min > terms[i].gap_max || terms[i].gap_max > ACM_CHAIN_GAP_MAX || terms[i].keyword_id >= n_keywords)
        return ACM_GPU_E_ARG;
      if (i == chain_ptr[c] && terms[i].gap_max != 0) /* (gap_min <= gap_max: both are 0) */
        return ACM_GPU_E_ARG;
    }
  return ACM_GPU_OK;
}

/* the total order of the output: end_pos ascending, length descending, chain id ascending */
static int
chain_out_cmp (const void *a, const void *b) {
  const ACMRecord *x = a, *y = b;
  if (x->end_pos != y->end_pos)
    return x->end_pos < y->end_pos ? -1 : 1;
  if (x->length != y->length)
    return x->length > y->length ? -1 : 1;
  return x->keyword_id < y->keyword_id ? -1 : x->keyword_id > y->keyword_id;
}

/* the first record of records[0 .. n) (canonical order) that ends at or behind end_pos */
static uint64_t
chain_first_at (const ACMRecord *records, uint64_t n, uint64_t end_pos) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (records[mid].end_pos < end_pos)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

#define CHAIN_NONE (~0ull)

int
acm_chains_records (const ACMRecord *records, uint64_t n, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                    const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, uint64_t n_keywords, ACMRecord *out,
                    uint64_t out_capacity, uint64_t *n_found) {
  if (!n_found || (n && !records) || (out_capacity && !out) || acm_chains_check (terms, chain_ptr, n_chains, n_keywords))
    return ACM_GPU_E_ARG;
  if (offsets) {
    if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
  }
  /* per chain the dynamic programme over its levels: best[i] = the greatest start of an embedding of the terms so far whose
   * last record is record i (CHAIN_NONE: there is none); the matches gather in `hits`, which grows as they come */
  uint64_t *best = malloc ((n ? n : 1) * sizeof *best), *prev = malloc ((n ? n : 1) * sizeof *prev);
  ACMRecord *hits = NULL;
  uint64_t found = 0, room = 0;
  int rc = best && prev ? ACM_GPU_OK : ACM_GPU_E_NOMEM;
  for (uint64_t c = 0; !rc && c < n_chains; c++) {
    for (uint64_t i = chain_ptr[c]; i < chain_ptr[c + 1]; i++) {
      const ACMChainTerm *term = &terms[i];
      uint64_t *swap = prev;
      prev = best;
      best = swap;
      for (uint64_t j = 0; j < n; j++) {
        const ACMRecord *r = &records[j];
        best[j] = CHAIN_NONE;
        if (r->keyword_id != term->keyword_id)
          continue;
        const uint64_t s = r->end_pos - pos_base + 1 - r->length;
        if (i == chain_ptr[c]) {
          best[j] = s;
          continue;
        }
        if (s < (uint64_t)term->gap_min + 1) /* the window [s - 1 - gap_max, s - 1 - gap_min] of ends is empty */
          continue;
        const uint64_t hi = s - 1 - term->gap_min, lo = s - 1 >= term->gap_max ? s - 1 - term->gap_max : 0;
        for (uint64_t w = chain_first_at (records, n, pos_base + lo); w < n && records[w].end_pos - pos_base <= hi; w++)
          if (records[w].keyword_id == terms[i - 1].keyword_id && prev[w] != CHAIN_NONE && (best[j] == CHAIN_NONE || prev[w] > best[j]))
            best[j] = prev[w];
      }
    }
    for (uint64_t j = 0; !rc && j < n; j++) {
      if (best[j] == CHAIN_NONE)
        continue;
      const uint64_t e = records[j].end_pos - pos_base, S = best[j];
      if (offsets) { /* one text holds S and e: the text of S, the largest with offsets[text] <= S, ends behind e */
        uint64_t lo = 0, hi = n_texts - 1;
        while (lo < hi) {
          const uint64_t mid = lo + (hi - lo + 1) / 2;
          if (offsets[mid] <= S)
            lo = mid;
          else
            hi = mid - 1;
        }
        if (e >= offsets[lo + 1])
          continue;
      }
      if (found == room) {
        room = room ? 2 * room : 256;
        ACMRecord *more = realloc (hits, room * sizeof *hits);
        if (!more) {
          rc = ACM_GPU_E_NOMEM;
          break;
        }
        hits = more;
      }
      hits[found++] = (ACMRecord){ records[j].end_pos, (uint32_t)(e + 1 - S), (uint32_t)c };
    }
  }
  free (best);
  free (prev);
  if (!rc) {
    *n_found = found;
    if (out && found > out_capacity)
      rc = ACM_GPU_E_OVERFLOW;
    else if (out) {
      if (found > 1)
        qsort (hits, found, sizeof *hits, chain_out_cmp);
      if (found)
        memcpy (out, hits, found * sizeof *hits);
    }
  }
  free (hits);
  return rc;
}

/* the check acm_scan_chains makes on every path: acm_chains_check against the machine's keywords */
int
acm_internal_chains_machine_check (ACMachine *m, const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains) {
  if (!m)
    return ACM_GPU_E_ARG;
  acm_internal_lock (m);
  const int rc = acm_chains_check (terms, chain_ptr, n_chains, m->nb_keywords);
  acm_internal_unlock (m);
  return rc;
}

/* acm_scan_chains on the host: the caller loop (from the root at every offset of a batch), then the sequential pass over what
 * it found -- what ACM_SCAN_PATH_CPU_LOOP runs.  The public call has checked the arguments. */
int
acm_internal_cpu_scan_chains (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                              const ACMChainTerm *terms, const uint64_t *chain_ptr, uint64_t n_chains, ACMRecord *out, uint64_t out_capacity,
                              uint64_t *n_found) {
  if (!m || !n_found)
    return ACM_GPU_E_ARG;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, offsets, n_texts, sym_bytes, NULL, &records, &found);
  if (!rc)
    rc = acm_chains_records (records, found, n_symbols, 0, offsets, n_texts, terms, chain_ptr, n_chains, acm_nb_keywords (m), out, out_capacity,
                             n_found);
  free (records);
  return rc;
}

/* ---- unordered keyword proximity (include/acm_near.h): the argument checks, the plain sequential NEAR of a record set in
 * canonical order, and acm_scan_near's host path. */
int
acm_near_check (const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups, uint64_t n_keywords) {
  if (!group_ptr || group_ptr[0] != 0 || n_groups >= (1ull << 31))
    return ACM_GPU_E_ARG;
  for (uint64_t g = 0; g < n_groups; g++)
    if (group_ptr[g] >= group_ptr[g + 1] || group_ptr[g + 1] - group_ptr[g] > ACM_NEAR_TERMS_MAX) /* decreasing, no term, too many */
      return ACM_GPU_E_ARG;
  if (group_ptr[n_groups] >= (1ull << 31) || (n_groups && (!terms || !groups)))
    return ACM_GPU_E_ARG;
  for (uint64_t g = 0; g < n_groups; g++) {
    const uint64_t m = group_ptr[g + 1] - group_ptr[g];
    if (groups[g].width == 0 || groups[g].width > ACM_NEAR_WIDTH_MAX || groups[g].need > m)
      return ACM_GPU_E_ARG;
    for (uint64_t i = group_ptr[g]; i < group_ptr[g + 1]; i++) {
      if (terms[i] >= n_keywords)
        return ACM_GPU_E_ARG;
      for (uint64_t j = group_ptr[g]; j < i; j++)
        if (terms[j] == terms[i])
          return ACM_GPU_E_ARG;
    }
  }
  return ACM_GPU_OK;
}

/* S* + 1 of the group whose terms are best[0 .. m) / at_end[0 .. m) (a start + 1, 0: none; at_end: of the record that ends at the
 * end in hand), by the closed form: the greatest over the anchors a of min (a_start, the (need - 1)-th greatest best_u, u != a) */
static uint64_t
near_best_window (const uint64_t *best, const uint64_t *at_end, uint64_t m, uint64_t need) {
  uint64_t top = 0;
  for (uint64_t a = 0; a < m; a++) {
    if (!at_end[a])
      continue;
    uint64_t S = at_end[a];
    if (need > 1) {
      uint64_t kth = 0; /* the (need - 1)-th greatest among the others: the one with need - 2 in front of it */
      for (uint64_t u = 0; u < m && !kth; u++) {
        if (u == a || !best[u])
          continue;
        uint64_t before = 0;
        for (uint64_t v = 0; v < m; v++)
          before += v != a && v != u && best[v] && (best[v] > best[u] || (best[v] == best[u] && v < u));
        if (before == need - 2)
          kth = best[u];
      }
      S = kth < S ? kth : S; /* (none: 0) */
    }
    top = S > top ? S : top;
  }
  return top;
}

int
acm_near_records (const ACMRecord *records, uint64_t n, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
                  const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups, uint64_t n_keywords,
                  ACMRecord *out, uint64_t out_capacity, uint64_t *n_found) {
  if (!n_found || (n && !records) || (out_capacity && !out) || acm_near_check (terms, group_ptr, groups, n_groups, n_keywords))
    return ACM_GPU_E_ARG;
  if (offsets) {
    if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  for (uint64_t j = 0; j < n; j++)
    if (record_breaks_contract (&records[j], pos_base, n_symbols))
      return ACM_GPU_E_ARG;
  /* the terms under their keywords (kw_ptr, kw_term: positions in terms[]), the group of a term, and one pass over the runs of
   * records of equal end: best[i] = the greatest start + 1 so far of term i's records, at_end[i] = that of the record of this
   * run (seen[i] = the run's number + 1 says whether it is this run's), hot[] the groups this run touched */
  const uint64_t n_terms = group_ptr[n_groups];
  uint64_t *kw_ptr = calloc (n_keywords + 2, sizeof *kw_ptr), *kw_term = malloc ((n_terms ? n_terms : 1) * sizeof *kw_term);
  uint64_t *group_of = malloc ((n_terms ? n_terms : 1) * sizeof *group_of), *best = calloc (n_terms ? n_terms : 1, sizeof *best);
  uint64_t *at_end = calloc (n_terms ? n_terms : 1, sizeof *at_end), *seen = calloc (n_terms ? n_terms : 1, sizeof *seen);
  uint64_t *hot = malloc ((n_groups ? n_groups : 1) * sizeof *hot), *hot_run = calloc (n_groups ? n_groups : 1, sizeof *hot_run);
  ACMRecord *hits = NULL;
  uint64_t found = 0, room = 0;
  int rc = kw_ptr && kw_term && group_of && best && at_end && seen && hot && hot_run ? ACM_GPU_OK : ACM_GPU_E_NOMEM;
  if (!rc) {
    for (uint64_t i = 0; i < n_terms; i++)
      kw_ptr[terms[i] + 2]++;
    for (uint64_t k = 0; k < n_keywords; k++)
      kw_ptr[k + 2] += kw_ptr[k + 1];
    for (uint64_t g = 0; g < n_groups; g++)
      for (uint64_t i = group_ptr[g]; i < group_ptr[g + 1]; i++) {
        kw_term[kw_ptr[terms[i] + 1]++] = i; /* (kw_ptr[k + 1] runs up to where kw_ptr[k + 2] began: kw_ptr[k .. k + 1] bound k's terms afterwards) */
        group_of[i] = g;
      }
  }
  uint64_t text = 0; /* the text of the run's end: ends ascend, so it only moves forward */
  for (uint64_t b = 0, run = 1; !rc && b < n; run++) {
    uint64_t c = b + 1, n_hot = 0;
    while (c < n && records[c].end_pos == records[b].end_pos)
      c++;
    const uint64_t e = records[b].end_pos - pos_base;
    for (uint64_t j = b; j < c; j++) {
      const ACMRecord *r = &records[j];
      if (r->keyword_id >= n_keywords)
        continue;
      const uint64_t s1 = e + 2 - r->length;
      for (uint64_t q = kw_ptr[r->keyword_id]; q < kw_ptr[r->keyword_id + 1]; q++) {
        const uint64_t i = kw_term[q], g = group_of[i];
        best[i] = s1 > best[i] ? s1 : best[i];
        at_end[i] = seen[i] == run && at_end[i] > s1 ? at_end[i] : s1;
        seen[i] = run;
        if (hot_run[g] != run) {
          hot_run[g] = run;
          hot[n_hot++] = g;
        }
      }
    }
    uint64_t begin = 0;
    if (offsets) {
      while (text + 1 < n_texts && offsets[text + 1] <= e)
        text++;
      begin = offsets[text];
    }
    for (uint64_t h = 0; !rc && h < n_hot; h++) {
      const uint64_t g = hot[h], t0 = group_ptr[g], m = group_ptr[g + 1] - t0;
      uint64_t anchors[ACM_NEAR_TERMS_MAX];
      for (uint64_t u = 0; u < m; u++)
        anchors[u] = seen[t0 + u] == run ? at_end[t0 + u] : 0;
      const uint64_t S1 = near_best_window (best + t0, anchors, m, groups[g].need ? groups[g].need : m);
      if (!S1 || S1 - 1 < begin || e + 1 - (S1 - 1) > groups[g].width)
        continue;
      if (found == room) {
        room = room ? 2 * room : 256;
        ACMRecord *more = realloc (hits, room * sizeof *hits);
        if (!more) {
          rc = ACM_GPU_E_NOMEM;
          break;
        }
        hits = more;
      }
      hits[found++] = (ACMRecord){ records[b].end_pos, (uint32_t)(e + 1 - (S1 - 1)), (uint32_t)g };
    }
    b = c;
  }
  free (kw_ptr);
  free (kw_term);
  free (group_of);
  free (best);
  free (at_end);
  free (seen);
  free (hot);
  free (hot_run);
  if (!rc) {
    *n_found = found;
    if (out && found > out_capacity)
      rc = ACM_GPU_E_OVERFLOW;
    else if (out) {
      if (found > 1)
        qsort (hits, found, sizeof *hits, chain_out_cmp);
      if (found)
        memcpy (out, hits, found * sizeof *hits);
    }
  }
  free (hits);
  return rc;
}

/* the check acm_scan_near makes on every path: acm_near_check against the machine's keywords */
int
acm_internal_near_machine_check (ACMachine *m, const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups) {
  if (!m)
    return ACM_GPU_E_ARG;
  acm_internal_lock (m);
  const int rc = acm_near_check (terms, group_ptr, groups, n_groups, m->nb_keywords);
  acm_internal_unlock (m);
  return rc;
}

/* acm_scan_near on the host: the caller loop (from the root at every offset of a batch), then the sequential pass over what it
 * found -- what ACM_SCAN_PATH_CPU_LOOP runs.  The public call has checked the arguments. */
int
acm_internal_cpu_scan_near (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                            const uint32_t *terms, const uint64_t *group_ptr, const ACMNearGroup *groups, uint64_t n_groups, ACMRecord *out,
                            uint64_t out_capacity, uint64_t *n_found) {
  if (!m || !n_found)
    return ACM_GPU_E_ARG;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, offsets, n_texts, sym_bytes, NULL, &records, &found);
  if (!rc)
    rc = acm_near_records (records, found, n_symbols, 0, offsets, n_texts, terms, group_ptr, groups, n_groups, acm_nb_keywords (m), out, out_capacity,
                           n_found);
  free (records);
  return rc;
}

/* ---- keywords with up to k mismatches (include/acm_gpu.h): the argument checks, the canonical cut, the plain sequential APPROX of a
 * record set in canonical order, and acm_scan_approx's host path. */
int
acm_approx_check (const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets,
                  uint64_t n_keywords) {
  if (!spell_off || !tgt_ptr || spell_off[0] != 0 || tgt_ptr[0] != 0 || n_targets >= (1ull << 31) || (n_targets && (!k || !terms)))
    return ACM_GPU_E_ARG;
  for (uint64_t w = 0; w < n_targets; w++) {
    if (tgt_ptr[w] >= tgt_ptr[w + 1]) /* decreasing, or a target without terms */
      return ACM_GPU_E_ARG;
    if (spell_off[w] >= spell_off[w + 1] || spell_off[w + 1] - spell_off[w] >= (1ull << 31) || k[w] > 255) /* decreasing, or L_w == 0 */
      return ACM_GPU_E_ARG;
  }
  if (tgt_ptr[n_targets] >= (1ull << 31))
    return ACM_GPU_E_ARG;
  for (uint64_t w = 0; w < n_targets; w++) {
    const uint64_t L = spell_off[w + 1] - spell_off[w];
    for (uint64_t i = tgt_ptr[w]; i < tgt_ptr[w + 1]; i++)
      if (terms[i].length == 0 || (uint64_t)terms[i].offset + terms[i].length > L || terms[i].keyword_id >= n_keywords)
        return ACM_GPU_E_ARG;
  }
  return ACM_GPU_OK;
}

int
acm_approx_split (uint64_t L, uint32_t k, uint32_t j, uint64_t *begin, uint64_t *end) {
  if (!begin || !end || L >= (1ull << 31) || L < (uint64_t)k + 1 || j > k)
    return ACM_GPU_E_ARG;
  *begin = (uint64_t)j * L / ((uint64_t)k + 1);
  *end = ((uint64_t)j + 1) * L / ((uint64_t)k + 1);
  return ACM_GPU_OK;
}

/* a term under its keyword: (target id, the term's index inside its target) */
struct apx_post {
  uint32_t keyword_id, target, j;
};

/* by keyword, then target id, then term index: the order of a keyword's postings */
static int
apx_post_cmp (const void *a, const void *b) {
  const struct apx_post *x = a, *y = b;
  if (x->keyword_id != y->keyword_id)
    return x->keyword_id < y->keyword_id ? -1 : 1;
  if (x->target != y->target)
    return x->target < y->target ? -1 : 1;
  return x->j < y->j ? -1 : x->j > y->j;
}

/* a match and its distance, so that the two are ordered together */
struct apx_hit {
  ACMRecord r;
  uint32_t d;
};

/* the output order: end_pos ascending, then length descending, then target id ascending */
static int
apx_hit_cmp (const void *a, const void *b) {
  const struct apx_hit *x = a, *y = b;
  if (x->r.end_pos != y->r.end_pos)
    return x->r.end_pos < y->r.end_pos ? -1 : 1;
  if (x->r.length != y->r.length)
    return x->r.length > y->r.length ? -1 : 1;
  return x->r.keyword_id < y->r.keyword_id ? -1 : x->r.keyword_id > y->r.keyword_id;
}

/* the tables of a call, as every entry point takes them */
struct apx_set {
  const unsigned char *spell;
  const uint64_t *spell_off;
  const uint32_t *k;
  const ACMPatternTerm *terms;
  const uint64_t *tgt_ptr;
  uint32_t sym_bytes;
  CMP_TYPE cmp; /* NULL: symbols compare bitwise */
  void *cmp_arg;
  const ACMTemplateSpec *tpl; /* TEMPLATES: the cells and the classes; NULL: every position is its spelling's symbol */
};

/* whether class c of a template set holds symbol x */
static int
tpl_class_has (const ACMTemplateSpec *T, uint32_t c, uint64_t x, uint32_t sb) {
  int in = 0;
  for (uint64_t r = T->cls_ptr[c]; !in && r < T->cls_ptr[c + 1]; r++)
    in = x >= words_symbol (T->ranges, 2 * r, sb) && x <= words_symbol (T->ranges, 2 * r + 1, sb);
  return (T->cls_flags[c] & ACM_TEMPLATE_NEGATED) ? !in : in;
}

/* whether target q->target matches with its term q->j seeded by record r (the term's keyword is the record's); *d = the mismatches */
static int
apx_matches (const ACMRecord *records, uint64_t n, const ACMRecord *r, const struct apx_post *q, const unsigned char *text, uint64_t n_symbols,
             uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts, const struct apx_set *A, uint64_t *S_out, uint32_t *d) {
  const uint64_t e = r->end_pos - pos_base, first = A->tgt_ptr[q->target], L = A->spell_off[q->target + 1] - A->spell_off[q->target];
  const ACMPatternTerm *term = &A->terms[first + q->j];
  if (r->length != term->length || (uint64_t)term->offset + term->length - 1 > e)
    return 0;
  const uint64_t S = e + 1 - term->length - term->offset;
  uint64_t t_hi = n_symbols; /* where the text of S ends */
  if (offsets) {
    if (!n_texts)
      return 0;
    uint64_t lo = 0, hi = n_texts - 1; /* the largest text with offsets[text] <= S */
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (offsets[mid] <= S)
        lo = mid;
      else
        hi = mid - 1;
    }
    t_hi = offsets[lo + 1];
  }
  if (S + L > t_hi)
    return 0;
  for (uint32_t i = 0; i < q->j; i++) { /* a term of lower index that seeds the same match emits it */
    const ACMPatternTerm *t = &A->terms[first + i];
    if (pat_has_record (records, n, pos_base + S + t->offset + t->length - 1, t->length, t->keyword_id))
      return 0;
  }
  const unsigned char *a = text + S * A->sym_bytes, *b = A->spell + A->spell_off[q->target] * A->sym_bytes;
  uint32_t miss = 0;
  const uint32_t *cells = A->tpl ? A->tpl->cells + A->spell_off[q->target] : NULL;
  for (uint64_t i = 0; i < L; i++) {
    int same;
    if (cells && cells[i] == ACM_TEMPLATE_ANY)
      same = 1;
    else if (cells && cells[i] != ACM_TEMPLATE_LITERAL) /* (a class cell: by value, whatever the comparator) */
      same = tpl_class_has (A->tpl, cells[i], words_symbol (a, i, A->sym_bytes), A->sym_bytes);
    else
      same = A->cmp ? A->cmp (a + i * A->sym_bytes, b + i * A->sym_bytes, A->cmp_arg) == 0
                    : memcmp (a + i * A->sym_bytes, b + i * A->sym_bytes, A->sym_bytes) == 0;
    if (!same && ++miss > A->k[q->target])
      return 0;
  }
  *S_out = S;
  *d = miss;
  return 1;
}

static int
approx_core (const ACMRecord *records, uint64_t n, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
             const struct apx_set *A, uint64_t n_targets, uint64_t n_keywords, ACMRecord *out, uint32_t *dist, uint64_t out_capacity,
             uint64_t *n_found) {
  if (!n_found || (n && !records) || (out_capacity && !out) || A->sym_bytes == 0 || (n_symbols && !text) || (n_targets && !A->spell) ||
      acm_approx_check (A->spell_off, A->k, A->terms, A->tgt_ptr, n_targets, n_keywords))
    return ACM_GPU_E_ARG;
  if (offsets) {
    if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
  }
  const uint64_t n_terms = A->tgt_ptr[n_targets];
  struct apx_post *post = malloc ((n_terms ? n_terms : 1) * sizeof *post);
  if (!post)
    return ACM_GPU_E_NOMEM;
  for (uint64_t w = 0; w < n_targets; w++)
    for (uint64_t i = A->tgt_ptr[w]; i < A->tgt_ptr[w + 1]; i++)
      post[i] = (struct apx_post){ A->terms[i].keyword_id, (uint32_t)w, (uint32_t)(i - A->tgt_ptr[w]) };
  qsort (post, n_terms, sizeof *post, apx_post_cmp);
  /* two passes over the records as seeds: the count, then -- when the matches fit -- the matches themselves */
  struct apx_hit *hit = NULL;
  uint64_t found = 0;
  for (int fill = 0; fill < 2; fill++) {
    found = 0;
    for (uint64_t j = 0; j < n; j++) {
      const ACMRecord *r = &records[j];
      uint64_t lo = 0, hi = n_terms; /* the keyword's first posting */
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (post[mid].keyword_id < r->keyword_id)
          lo = mid + 1;
        else
          hi = mid;
      }
      for (uint64_t q = lo; q < n_terms && post[q].keyword_id == r->keyword_id; q++) {
        uint64_t S = 0;
        uint32_t d = 0;
        if (!apx_matches (records, n, r, &post[q], text, n_symbols, pos_base, offsets, n_texts, A, &S, &d))
          continue;
        if (fill) {
          const uint64_t L = A->spell_off[post[q].target + 1] - A->spell_off[post[q].target];
          hit[found] = (struct apx_hit){ { pos_base + S + L - 1, (uint32_t)L, post[q].target }, d };
        }
        found++;
      }
    }
    if (!out || found > out_capacity || found == 0) /* the call only counts, or the matches have no room */
      break;
    if (!fill && !(hit = malloc (found * sizeof *hit))) {
      free (post);
      return ACM_GPU_E_NOMEM;
    }
  }
  free (post);
  *n_found = found;
  if (out && found <= out_capacity && found) {
    qsort (hit, found, sizeof *hit, apx_hit_cmp); /* the seeds lie anywhere inside their targets */
    for (uint64_t i = 0; i < found; i++) {
      out[i] = hit[i].r;
      if (dist)
        dist[i] = hit[i].d;
    }
  }
  free (hit);
  return out && found > out_capacity ? ACM_GPU_E_OVERFLOW : ACM_GPU_OK;
}

int
acm_approx_records (const ACMRecord *records, uint64_t n, const void *text, uint32_t sym_bytes, uint64_t n_symbols, uint64_t pos_base,
                    const uint64_t *offsets, uint64_t n_texts, const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                    const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets, uint64_t n_keywords, ACMRecord *out, uint32_t *dist,
                    uint64_t out_capacity, uint64_t *n_found) {
  const struct apx_set A = { spell_data, spell_off, k, terms, tgt_ptr, sym_bytes, NULL, NULL, NULL };
  return approx_core (records, n, text, n_symbols, pos_base, offsets, n_texts, &A, n_targets, n_keywords, out, dist, out_capacity, n_found);
}

/* the checks acm_scan_approx makes on every path: acm_approx_check against the machine's keywords, and every term's keyword is
 * spelled as the term's piece of its target (by the machine's comparator over symbols of sym_bytes bytes) */
int
acm_internal_approx_machine_check (ACMachine *m, uint32_t sym_bytes, const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                                   const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets) {
  if (!m || !sym_bytes || (n_targets && !spell_data))
    return ACM_GPU_E_ARG;
  acm_internal_lock (m);
  int rc = acm_approx_check (spell_off, k, terms, tgt_ptr, n_targets, m->nb_keywords);
  for (uint64_t w = 0; !rc && w < n_targets; w++)
    for (uint64_t i = tgt_ptr[w]; !rc && i < tgt_ptr[w + 1]; i++) {
      const struct _ac_state *s = m->keywords[terms[i].keyword_id];
      if (s->depth != terms[i].length) {
        rc = ACM_GPU_E_ARG;
        break;
      }
      const unsigned char *piece = (const unsigned char *)spell_data + (spell_off[w] + terms[i].offset) * sym_bytes;
      for (uint32_t at = terms[i].length; !rc && at-- > 0; s = s->parent)
        if (m->cmp (s->letter, piece + (size_t)at * sym_bytes, m->cmp_arg) != 0)
          rc = ACM_GPU_E_ARG;
    }
  acm_internal_unlock (m);
  return rc;
}

/* acm_scan_approx on the host: the caller loop (from the root at every offset of a batch), then the sequential pass over what it
 * found, with symbols compared by the machine's comparator -- what ACM_SCAN_PATH_CPU_LOOP runs.  The public call has checked the
 * arguments. */
int
acm_internal_cpu_scan_approx (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                              const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms,
                              const uint64_t *tgt_ptr, uint64_t n_targets, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  if (!m || !n_found)
    return ACM_GPU_E_ARG;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, offsets, n_texts, sym_bytes, NULL, &records, &found);
  if (!rc) {
    const struct apx_set A = { spell_data, spell_off, k, terms, tgt_ptr, sym_bytes, m->cmp, m->cmp_arg, NULL };
    rc = approx_core (records, found, text, n_symbols, 0, offsets, n_texts, &A, n_targets, acm_nb_keywords (m), out, dist, out_capacity, n_found);
  }
  free (records);
  return rc;
}

/* ---- keyword templates with symbol classes (include/acm_gpu.h): the argument checks, the canonical cut, the plain sequential TEMPLATES
 * and acm_scan_templates' host path.  The set, the postings, the hits and the pass are APPROX's; apx_matches takes the cells. */
int
acm_templates_check (const ACMTemplateSpec *T, uint32_t sym_bytes, uint64_t n_keywords) {
  if (!T || (sym_bytes != 1 && sym_bytes != 2 && sym_bytes != 4 && sym_bytes != 8) || T->n_classes >= ACM_TEMPLATE_ANY ||
      (T->n_classes && (!T->cls_ptr || !T->cls_flags)) || (T->cls_ptr && T->cls_ptr[0] != 0))
    return ACM_GPU_E_ARG;
  for (uint64_t c = 0; c < T->n_classes; c++) {
    if (T->cls_ptr[c] > T->cls_ptr[c + 1] || T->cls_ptr[c + 1] - T->cls_ptr[c] > ACM_TEMPLATE_MAX_RANGES || (T->cls_ptr[c + 1] && !T->ranges))
      return ACM_GPU_E_ARG;
    for (uint64_t r = T->cls_ptr[c]; r < T->cls_ptr[c + 1]; r++)
      if (words_symbol (T->ranges, 2 * r, sym_bytes) > words_symbol (T->ranges, 2 * r + 1, sym_bytes))
        return ACM_GPU_E_ARG;
  }
  if (acm_approx_check (T->spell_off, T->k, T->terms, T->tgt_ptr, T->n_templates, n_keywords) || (T->n_templates && !T->cells))
    return ACM_GPU_E_ARG;
  for (uint64_t i = 0; i < T->spell_off[T->n_templates]; i++)
    if (T->cells[i] < ACM_TEMPLATE_ANY && T->cells[i] >= T->n_classes)
      return ACM_GPU_E_ARG;
  for (uint64_t w = 0; w < T->n_templates; w++)
    for (uint64_t i = T->tgt_ptr[w]; i < T->tgt_ptr[w + 1]; i++) /* a piece is an exact keyword: literal cells only */
      for (uint32_t at = 0; at < T->terms[i].length; at++)
        if (T->cells[T->spell_off[w] + T->terms[i].offset + at] != ACM_TEMPLATE_LITERAL)
          return ACM_GPU_E_ARG;
  return ACM_GPU_OK;
}

/* the pieces of q cells that the literal runs of a template give: sum over runs of floor (run / q); with `j`, where piece j begins */
static uint64_t
tpl_pieces (const uint32_t *cells, uint64_t L, uint64_t q, const uint32_t *j, uint64_t *offset) {
  uint64_t pieces = 0;
  for (uint64_t i = 0; i < L;) {
    if (cells[i] != ACM_TEMPLATE_LITERAL) {
      i++;
      continue;
    }
    uint64_t run = i;
    while (run < L && cells[run] == ACM_TEMPLATE_LITERAL)
      run++;
    const uint64_t here = (run - i) / q;
    if (j && *j >= pieces && *j < pieces + here)
      *offset = i + (*j - pieces) * q;
    pieces += here;
    i = run;
  }
  return pieces;
}

int
acm_templates_split (const uint32_t *cells, uint64_t L, uint32_t k, uint32_t j, uint64_t *offset, uint64_t *length) {
  if (!cells || !offset || !length || L == 0 || L >= (1ull << 31) || j > k || tpl_pieces (cells, L, 1, NULL, NULL) < (uint64_t)k + 1)
    return ACM_GPU_E_ARG;
  uint64_t q = 1; /* the largest length that still gives k + 1 pieces (the number of pieces does not grow with q) */
  while (q < L && tpl_pieces (cells, L, q + 1, NULL, NULL) >= (uint64_t)k + 1)
    q++;
  (void)tpl_pieces (cells, L, q, &j, offset);
  *length = q;
  return ACM_GPU_OK;
}

int
acm_templates_records (const ACMRecord *records, uint64_t n, const void *text, uint32_t sym_bytes, uint64_t n_symbols, uint64_t pos_base,
                       const uint64_t *offsets, uint64_t n_texts, const ACMTemplateSpec *T, uint64_t n_keywords, ACMRecord *out, uint32_t *dist,
                       uint64_t out_capacity, uint64_t *n_found) {
  if (acm_templates_check (T, sym_bytes, n_keywords))
    return ACM_GPU_E_ARG;
  const struct apx_set A = { T->spell_data, T->spell_off, T->k, T->terms, T->tgt_ptr, sym_bytes, NULL, NULL, T };
  return approx_core (records, n, text, n_symbols, pos_base, offsets, n_texts, &A, T->n_templates, n_keywords, out, dist, out_capacity, n_found);
}

/* the checks acm_scan_templates makes on every path: acm_templates_check against the machine's keywords, and acm_scan_approx's on the
 * terms (they stand on literal cells, so their pieces are spelled in spell_data) */
int
acm_internal_templates_machine_check (ACMachine *m, uint32_t sym_bytes, const ACMTemplateSpec *T) {
  if (!m || !T)
    return ACM_GPU_E_ARG;
  acm_internal_lock (m);
  const int rc = acm_templates_check (T, sym_bytes, m->nb_keywords);
  acm_internal_unlock (m);
  return rc ? rc : acm_internal_approx_machine_check (m, sym_bytes, T->spell_data, T->spell_off, T->k, T->terms, T->tgt_ptr, T->n_templates);
}

/* acm_scan_templates on the host: acm_internal_cpu_scan_approx with the cells; literal cells by the comparator, class cells by value */
int
acm_internal_cpu_scan_templates (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                                 const ACMTemplateSpec *T, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  if (!m || !n_found || !T)
    return ACM_GPU_E_ARG;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, offsets, n_texts, sym_bytes, NULL, &records, &found);
  if (!rc) {
    const struct apx_set A = { T->spell_data, T->spell_off, T->k, T->terms, T->tgt_ptr, sym_bytes, m->cmp, m->cmp_arg, T };
    rc = approx_core (records, found, text, n_symbols, 0, offsets, n_texts, &A, T->n_templates, acm_nb_keywords (m), out, dist, out_capacity, n_found);
  }
  free (records);
  return rc;
}

/* ---- keywords within edit distance k (include/acm_gpu.h): the two further conditions on the budgets, the plain sequential EDIT of a
 * record set in canonical order, and acm_scan_edit's host path.  The set, the postings and the hits are APPROX's (apx_set, apx_post,
 * apx_hit); what differs is the verification: a seed fixes a window of ends, not one start. */
#define EDIT_MAX_K 15u
#define EDIT_INF 0xFFFFFFFFu

/* the conditions the edit calls add to acm_approx_check: k[w] <= 15 and k[w] < L_w */
static int
edit_budgets_check (const uint64_t *spell_off, const uint32_t *k, uint64_t n_targets) {
  for (uint64_t w = 0; w < n_targets; w++)
    if (k[w] > EDIT_MAX_K || k[w] >= spell_off[w + 1] - spell_off[w])
      return ACM_GPU_E_ARG;
  return ACM_GPU_OK;
}

int
acm_edit_check (const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets,
                uint64_t n_keywords) {
  if (acm_approx_check (spell_off, k, terms, tgt_ptr, n_targets, n_keywords))
    return ACM_GPU_E_ARG;
  return edit_budgets_check (spell_off, k, n_targets);
}

/* the hits of a call, grown as the seeds are walked */
struct edit_hits {
  struct apx_hit *hit;
  uint64_t n, room;
};

static int
edit_hits_push (struct edit_hits *H, uint64_t end_pos, uint32_t length, uint32_t target, uint32_t d) {
  if (H->n == H->room) {
    const uint64_t room = H->room ? 2 * H->room : 64;
    struct apx_hit *grown = realloc (H->hit, room * sizeof *grown);
    if (!grown)
      return ACM_GPU_E_NOMEM;
    H->hit = grown;
    H->room = room;
  }
  H->hit[H->n++] = (struct apx_hit){ { end_pos, length, target }, d };
  return ACM_GPU_OK;
}

/* What one seed gives: record r is term q->j of target q->target (the term's keyword is the record's).  The ends it can seed are
 * [e0, e1]; the banded dynamic programme over the diagonals [e0 + 1 - L - k, e1 + 1 - L + k] gives (D, s*) at every such end whose
 * D is within the budget.  Cell (i, c): i symbols of the target matched, the text consumed up to c; diagonal index d = c - i - B.
 * A cell is cost << 6 | (63 - d0) with d0 the diagonal index its path began on in row 0, so that one minimum takes the least cost
 * and then the largest start; cells above k, left of lo and right of e1 + 1 do not exist (EDIT_INF). */
static int
edit_window (const ACMRecord *r, const struct apx_post *q, const unsigned char *text, uint64_t n_symbols, uint64_t pos_base,
             const uint64_t *offsets, uint64_t n_texts, const struct apx_set *A, struct edit_hits *H) {
  const uint64_t eq = r->end_pos - pos_base, L = A->spell_off[q->target + 1] - A->spell_off[q->target];
  const ACMPatternTerm *term = &A->terms[A->tgt_ptr[q->target] + q->j];
  const uint32_t k = A->k[q->target], sb = A->sym_bytes;
  if (r->length != term->length)
    return ACM_GPU_OK;
  uint64_t t_lo = 0, t_hi = n_symbols; /* the text of the record's end */
  if (offsets) {
    if (!n_texts)
      return ACM_GPU_OK;
    uint64_t lo = 0, hi = n_texts - 1; /* the largest text with offsets[text] <= eq */
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      if (offsets[mid] <= eq)
        lo = mid;
      else
        hi = mid - 1;
    }
    t_lo = offsets[lo];
    t_hi = offsets[lo + 1];
  }
  if (eq + 1 < t_lo + term->length) /* the piece begins in front of its text: a record that spans a cut */
    return ACM_GPU_OK;
  const uint64_t behind = L - term->offset - term->length; /* the symbols of the target behind the piece */
  const uint64_t e0 = eq + (behind > k ? behind - k : 0), e1 = eq + behind + k < t_hi - 1 ? eq + behind + k : t_hi - 1;
  if (e0 > e1)
    return ACM_GPU_OK;
  const int64_t B = (int64_t)e0 + 1 - (int64_t)L - (int64_t)k, c_lo = (int64_t)t_lo, c_hi = (int64_t)e1 + 1;
  const uint32_t nd = (uint32_t)(e1 - e0) + 2 * k + 1; /* <= 4 k + 1 <= 61 */
  const unsigned char *spell = A->spell + A->spell_off[q->target] * sb;
  uint32_t row_a[64], row_b[64], *prev = row_a, *cur = row_b;
  for (uint32_t d = 0; d < nd; d++)
    prev[d] = B + d >= c_lo && B + d <= c_hi ? 63 - d : EDIT_INF;
  for (uint64_t i = 1; i <= L; i++) {
    int any = 0;
    for (uint32_t d = 0; d < nd; d++) {
      const int64_t c = B + (int64_t)d + (int64_t)i;
      uint32_t v = EDIT_INF;
      if (c >= c_lo && c <= c_hi) {
        if (c > c_lo && prev[d] != EDIT_INF) {
          const unsigned char *a = text + (uint64_t)(c - 1) * sb, *b = spell + (i - 1) * sb;
          const int same = A->cmp ? A->cmp (a, b, A->cmp_arg) == 0 : memcmp (a, b, sb) == 0;
          v = prev[d] + (same ? 0 : 64);
        }
        if (d + 1 < nd && prev[d + 1] != EDIT_INF && prev[d + 1] + 64 < v)
          v = prev[d + 1] + 64;
        if (d > 0 && cur[d - 1] != EDIT_INF && cur[d - 1] + 64 < v)
          v = cur[d - 1] + 64;
        if (v != EDIT_INF && (v >> 6) > k)
          v = EDIT_INF;
      }
      cur[d] = v;
      any |= v != EDIT_INF;
    }
    if (!any) /* Ukkonen's cut-off: no cell of this row is within the budget, so none behind it is */
      return ACM_GPU_OK;
    uint32_t *t = prev;
    prev = cur;
    cur = t;
  }
  for (uint32_t d = k; d <= k + (uint32_t)(e1 - e0); d++)
    if (prev[d] != EDIT_INF) {
      const uint32_t d0 = 63 - (prev[d] & 63);
      if (edit_hits_push (H, pos_base + e0 - k + d, (uint32_t)(L + d - d0), q->target, prev[d] >> 6))
        return ACM_GPU_E_NOMEM;
    }
  return ACM_GPU_OK;
}

/* approx_core's argument walk, then every seed's window; the hits are ordered, and what several seeds reached is kept once */
static int
edit_core (const ACMRecord *records, uint64_t n, const void *text, uint64_t n_symbols, uint64_t pos_base, const uint64_t *offsets, uint64_t n_texts,
           const struct apx_set *A, uint64_t n_targets, uint64_t n_keywords, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  if (!n_found || (n && !records) || (out_capacity && !out) || A->sym_bytes == 0 || (n_symbols && !text) || (n_targets && !A->spell) ||
      acm_edit_check (A->spell_off, A->k, A->terms, A->tgt_ptr, n_targets, n_keywords))
    return ACM_GPU_E_ARG;
  if (offsets) {
    if (offsets[0] != 0 || offsets[n_texts] != n_symbols)
      return ACM_GPU_E_ARG;
    for (uint64_t t = 0; t < n_texts; t++)
      if (offsets[t] > offsets[t + 1])
        return ACM_GPU_E_ARG;
  }
  for (uint64_t j = 0; j < n; j++) {
    const ACMRecord *r = &records[j];
    if (record_breaks_contract (r, pos_base, n_symbols))
      return ACM_GPU_E_ARG;
  }
  const uint64_t n_terms = A->tgt_ptr[n_targets];
  struct apx_post *post = malloc ((n_terms ? n_terms : 1) * sizeof *post);
  if (!post)
    return ACM_GPU_E_NOMEM;
  for (uint64_t w = 0; w < n_targets; w++)
    for (uint64_t i = A->tgt_ptr[w]; i < A->tgt_ptr[w + 1]; i++)
      post[i] = (struct apx_post){ A->terms[i].keyword_id, (uint32_t)w, (uint32_t)(i - A->tgt_ptr[w]) };
  qsort (post, n_terms, sizeof *post, apx_post_cmp);
  struct edit_hits H = { NULL, 0, 0 };
  int rc = ACM_GPU_OK;
  for (uint64_t j = 0; !rc && j < n; j++) {
    const ACMRecord *r = &records[j];
    uint64_t lo = 0, hi = n_terms; /* the keyword's first posting */
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (post[mid].keyword_id < r->keyword_id)
        lo = mid + 1;
      else
        hi = mid;
    }
    for (uint64_t q = lo; !rc && q < n_terms && post[q].keyword_id == r->keyword_id; q++)
      rc = edit_window (r, &post[q], text, n_symbols, pos_base, offsets, n_texts, A, &H);
  }
  free (post);
  if (rc) {
    free (H.hit);
    return rc;
  }
  /* (w, e) reached from several seeds has one D and one s*, so its hits are equal and stand side by side in the order */
  uint64_t found = 0;
  if (H.n) {
    qsort (H.hit, H.n, sizeof *H.hit, apx_hit_cmp);
    for (uint64_t i = 0; i < H.n; i++)
      if (!found || H.hit[i].r.end_pos != H.hit[found - 1].r.end_pos || H.hit[i].r.keyword_id != H.hit[found - 1].r.keyword_id ||
          H.hit[i].r.length != H.hit[found - 1].r.length)
        H.hit[found++] = H.hit[i];
  }
  *n_found = found;
  if (out && found <= out_capacity)
    for (uint64_t i = 0; i < found; i++) {
      out[i] = H.hit[i].r;
      if (dist)
        dist[i] = H.hit[i].d;
    }
  free (H.hit);
  return out && found > out_capacity ? ACM_GPU_E_OVERFLOW : ACM_GPU_OK;
}

int
acm_edit_records (const ACMRecord *records, uint64_t n, const void *text, uint32_t sym_bytes, uint64_t n_symbols, uint64_t pos_base,
                  const uint64_t *offsets, uint64_t n_texts, const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                  const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets, uint64_t n_keywords, ACMRecord *out, uint32_t *dist,
                  uint64_t out_capacity, uint64_t *n_found) {
  const struct apx_set A = { spell_data, spell_off, k, terms, tgt_ptr, sym_bytes, NULL, NULL, NULL };
  return edit_core (records, n, text, n_symbols, pos_base, offsets, n_texts, &A, n_targets, n_keywords, out, dist, out_capacity, n_found);
}

/* the checks acm_scan_edit makes on every path: acm_scan_approx's, plus the two conditions on the budgets */
int
acm_internal_edit_machine_check (ACMachine *m, uint32_t sym_bytes, const void *spell_data, const uint64_t *spell_off, const uint32_t *k,
                                 const ACMPatternTerm *terms, const uint64_t *tgt_ptr, uint64_t n_targets) {
  if (acm_internal_approx_machine_check (m, sym_bytes, spell_data, spell_off, k, terms, tgt_ptr, n_targets))
    return ACM_GPU_E_ARG;
  return edit_budgets_check (spell_off, k, n_targets);
}

/* acm_scan_edit on the host: acm_internal_cpu_scan_approx with the sequential EDIT behind the caller loop */
int
acm_internal_cpu_scan_edit (ACMachine *m, const void *text, uint64_t n_symbols, uint32_t sym_bytes, const uint64_t *offsets, uint64_t n_texts,
                            const void *spell_data, const uint64_t *spell_off, const uint32_t *k, const ACMPatternTerm *terms,
                            const uint64_t *tgt_ptr, uint64_t n_targets, ACMRecord *out, uint32_t *dist, uint64_t out_capacity, uint64_t *n_found) {
  if (!m || !n_found)
    return ACM_GPU_E_ARG;
  ACMRecord *records;
  uint64_t found = 0;
  int rc = cpu_scan_grown (m, text, n_symbols, offsets, n_texts, sym_bytes, NULL, &records, &found);
  if (!rc) {
    const struct apx_set A = { spell_data, spell_off, k, terms, tgt_ptr, sym_bytes, m->cmp, m->cmp_arg, NULL };
    rc = edit_core (records, found, text, n_symbols, 0, offsets, n_texts, &A, n_targets, acm_nb_keywords (m), out, dist, out_capacity, n_found);
  }
  free (records);
  return rc;
}
