"""Shared by tests/test_growth_cpu.py and tests/test_growth_gpu.py: the ways a plan can come to hold a dictionary
(acm_gpu_plan_update, include/acm_gpu.h), as plan makers that fit stream_cases.Features (..., make_plan, ...).

Every maker builds a SHADOW machine and inserts the final machine's keywords into it in the same order, in the groups
steps () names, so that keyword ids are the final machine's; the plan it returns reports all K keywords.

    built       the control: one plan of everything
    born_empty  the plan of the empty machine, then one update with everything: all facts come from the delta
    stepwise    born empty, then three updates of a third each with a scan on the null stream between them: a delta
                replaced twice, its forerunners waiting in the plan's retired list and then destroyed
    outgrown    the base is the first keyword alone, the rest arrive as the delta: the delta is longer, has more outputs
                per state and other symbols than the base (tests/test_growth_cpu.py)
    merged      outgrown without the last keyword, the compiled sets made on that plan, then an update with the last
                keyword under ACM_GPU_DELTA=0: one plan of everything behind the same handle, with sets made before it
    gram_base   the 4-gram kind of tests/tally_cases.py (20,000 synthetic keywords) as the base, the sets' pieces as its
                delta: what a caller gets who compiles a set on a live 4-gram plan

The byte dictionary is batch_cases.KEYWORDS plus the pieces the sets of a Features add, plus TRAILING."""
import os

import numpy as np

import aho_corasick_1975_amd as acm
from tests import family_stream_cases as fc
from tests import stream_cases as sc
from tests.batch_cases import KEYWORDS, packed_batch
from tests.cases import build_pair
from tests.tally_cases import kind, planted

SHAPES = ["built", "born_empty", "stepwise", "outgrown", "merged", "gram_base"]
N_SYMBOLS = 4096
GRAM_KEYWORDS = 20000                                    # synthetic keywords of the 4-gram base (a few are equal: somewhat fewer ids)
TRAILING = b"ir."                                        # the last keyword: no set refers to it, and both batches hold it
# the compiled sets a merged plan gets in front of its merging update (flows are made after growth everywhere: a flows
# object made before a longer keyword arrived is ACM_GPU_E_ARG by the header)
SETS_FIRST = ["rules", "patterns", "chains", "approx", "edit", "templates"]


def batch(seed):
    """N_SYMBOLS symbols made of the keywords and of letters around them -- `s` and `h` only inside keywords, so that the
    one-symbol keywords leave room for the records of a batch in the room of a Features -- under the offsets of
    tests/batch_cases.py::packed_batch: 37 texts, empty ones at either end, one of 700 symbols"""
    rng = np.random.default_rng(seed)
    words = [b"she", b"he", b"hers", b"s", b"ir.", b"e", b"i", b"r", b" ", b".", b" he ", b" she."]
    p = np.array([2.0, 2.0, 0.6, 1.0, 1.0, 4.0, 24.0, 24.0, 30.0, 8.0, 0.7, 0.5])
    picks = rng.choice(len(words), size=N_SYMBOLS, p=p / p.sum())
    text = np.frombuffer(b"".join(words[i] for i in picks)[:N_SYMBOLS], np.uint8).copy()
    assert text.size == N_SYMBOLS
    return text, packed_batch(N_SYMBOLS)[1]


def keywords_of(m):
    """the machine's keywords in id order, as arrays of its symbol type"""
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[m.sym_size]
    return [np.array(m.keyword(k)[0], dt) for k in range(m.nb_keywords)]


def steps(shape, n_keywords, base=None):
    """the groups of keyword ids a shape's shadow machine takes one after the other: the first is what the plan is made of
    (empty: the plan of the empty machine), every further one arrives by an update.  base: the keywords of gram_base's base"""
    K = n_keywords
    ids = list(range(K))
    if shape == "built":
        return [ids]
    if shape == "born_empty":
        return [[], ids]
    if shape == "stepwise":
        return [[], ids[:K // 3], ids[K // 3:2 * K // 3], ids[2 * K // 3:]]
    if shape == "outgrown":
        return [ids[:1], ids[1:]]
    if shape == "merged":
        return [ids[:1], ids[1:K - 1], ids[K - 1:]]
    assert shape == "gram_base" and K > base > GRAM_KEYWORDS - 100, (shape, K, base)
    return [ids[:base], ids[base:]]


def shadow_of(keywords, groups, sym_size=1, new_machine=None):
    """a machine with the keywords of `groups` inserted in order (the CPU half of a maker)"""
    m = new_machine() if new_machine is not None else acm.Machine(sym_size)
    for g in groups:
        for k in g:
            m.add_keyword(keywords[k])
    return m


class Grown:
    """a plan that grows group by group; keeps its shadow machine alive"""

    def __init__(self, keywords, groups, device=0, sym_size=1, new_machine=None, plan_of=None):
        self.keywords, self.groups = keywords, [list(g) for g in groups]
        self.m = new_machine() if new_machine is not None else acm.Machine(sym_size)
        self._add(self.groups[0])
        self.plan = plan_of(self.m, device) if plan_of is not None else self.m.plan(device)
        self.done = 1

    def _add(self, group):
        if len(group) >= 1000 and self.m.sym_size == 1:  # (the 4-gram base: packed, as tests/tally_cases.py makes it)
            data = np.concatenate([self.keywords[k] for k in group])
            off = np.concatenate([[0], np.cumsum([self.keywords[k].size for k in group])]).astype(np.uint32)
            self.m.add_keywords_packed(data, off)
            return
        for k in group:
            self.m.add_keyword(self.keywords[k])

    def step(self, delta=True):
        """the next group into the machine, and the update; delta False: under ACM_GPU_DELTA=0, a rebuild of everything"""
        self._add(self.groups[self.done])
        self.done += 1
        before = os.environ.get("ACM_GPU_DELTA")
        if not delta:
            os.environ["ACM_GPU_DELTA"] = "0"
        try:
            self.plan.update(self.m)
        finally:
            if not delta:
                if before is None:
                    del os.environ["ACM_GPU_DELTA"]
                else:
                    os.environ["ACM_GPU_DELTA"] = before
        return self.plan.info


def maker(shape, m, probe=None, keep=None, base=None):
    """make_plan (device) for a Features over the byte machine `m` (read when the plan is made: the sets' pieces are in by
    then).  probe (plan): a scan on the null stream, run between the updates of `stepwise`.  keep: a list the Grown goes
    into (merged: its last step is last_step ())."""
    def make_plan(device):
        kws = keywords_of(m)
        K = len(kws)
        g = Grown(kws, steps(shape, K, base), device)
        if keep is not None:
            keep.append(g)
        first = len(g.groups[0])
        if shape == "gram_base":
            assert g.plan.info.kernel == 5, g.plan.describe()
        if shape == "merged":
            info = g.step()
            assert info.delta_keywords == K - 2 and info.merges == 0, g.plan.describe()
            return g.plan                                # (the merging update: last_step)
        while g.done < len(g.groups):
            info = g.step()
            covered = sum(len(x) for x in g.groups[:g.done])
            assert info.delta_keywords == covered - first and info.merges == 0, (shape, g.plan.describe())
            if shape == "stepwise":
                probe(g.plan)
        if shape == "born_empty":
            assert g.plan.info.delta_keywords == K and g.plan.info.merges == 0
        if shape == "gram_base":
            assert g.plan.info.kernel == 5 and g.plan.info.delta_keywords == K - base > 0, g.plan.describe()
        g.plan.shadow = g                                # (the plan does not own its machine)
        return g.plan
    return make_plan


def last_step(keep):
    """merged: the sets compiled on the plan of K - 1 keywords, then the update that rebuilds everything"""
    def run(f):
        g = keep[-1]
        for family in SETS_FIRST:
            f.handle(family)
        fc.near_handle(f)
        fc.score_handle(f)
        info = g.step(delta=False)
        assert info.merges == 1 and info.delta_keywords == 0, g.plan.describe()
        g.plan.shadow = g
    return run


# ---------------------------------------------------------------------------------------------- other symbol sizes and class plans
HOWS = {2: ["starts1", "starts2"], 4: ["starts1", "starts2"], 8: ["outgrown"]}


def grown(keywords, how, sym_size=1, new_machine=None, plan_of=None, probe=None):
    """a Grown of `keywords` (arrays of symbols, in id order): the plan of the first keyword, then
        starts1   one update with the rest: a start-parallel plan (2- and 4-byte symbols) is edited in place, and its
                  first edit moves its tables out of the blob they were created in;
        starts2   the rest in two updates, probe (plan) -- a scan -- between them: the second edit patches the tables the
                  first one moved;
        outgrown  one update with the rest, which are the delta of any other kind of plan: of 8-byte symbols (the delta's
                  intern table holds symbols the base's lacks) or of comparator classes (the delta's class table has
                  members the base never saw)."""
    K = len(keywords)
    rest = list(range(1, K))
    groups = [[0], rest[:len(rest) // 2], rest[len(rest) // 2:]] if how == "starts2" else [[0], rest]
    assert all(groups)
    g = Grown(keywords, groups, 0, sym_size, new_machine, plan_of)
    in_place = how in ("starts1", "starts2")
    assert not in_place or g.plan.info.kernel == 4, g.plan.describe()
    while g.done < len(groups):
        info = g.step()
        if in_place:
            assert info.kernel == 4 and info.delta_keywords == 0 and info.merges == 0, g.plan.describe()
        else:
            assert info.delta_keywords == K - 1 and info.merges == 0, g.plan.describe()
        if probe is not None and g.done < len(groups):
            probe(g.plan)
    assert g.plan.tally_keywords == K
    g.plan.shadow = g
    return g


def features(torch, shape):
    """the Features of a shape; torch None: without a plan, for the expected values alone"""
    keep = []

    def probe(plan):
        assert int(plan.count(torch.from_numpy(real).cuda()).item()) >= 0
        plan.status()
    if shape == "gram_base":
        m, o, text, _, _, _ = kind("gram", None, None)
        real, decoy, off = planted(text[:N_SYMBOLS], 77), planted(text[2 * N_SYMBOLS:3 * N_SYMBOLS], 78), batch(0)[1]
        base = m.nb_keywords
        f = sc.Features(torch, m, o, maker(shape, m, probe, keep, base), real, decoy, off, word_ranges=((0x61, 0x6D),))
        f.base_keywords = base
        return f
    (real, off), (decoy, _) = batch(81), batch(82)
    m, o = build_pair(KEYWORDS, 1)
    return sc.Features(torch, m, o, maker(shape, m, probe, keep), real, decoy, off, trailing=TRAILING,
                       last_step=last_step(keep) if shape == "merged" else None)


# ---------------------------------------------------------------------------------------------- the entry points of the sweep
EXCLUDED = {
    "acm_gpu_synth_text": "the bench's text generator takes no plan: nothing a plan's growth could change",
    "acm_gpu_comm_gather_records": sc.EXCLUDED["acm_gpu_comm_gather_records"],
}
ENTRIES = sc.PLAIN + sc.FEATURES + sc.ANCHORED + fc.ENTRIES


def anchored_expected(f, which):
    """{entry: expected outputs} of the two anchored entry points over the Features' own batch: ANCHORED (prefixes) and
    LOOKUP by their definitions (tests/anchored_cases.py) over the oracle's records"""
    from tests import anchored_cases as ac
    text = f.real if which == "real" else f.decoy
    rec, text_of = ac.batch_records(f.o, text, f.off)
    r, tid, first = ac.anchored(rec, f.off, ac.PREFIXES, text_of)
    whole, prefix, length = ac.lookup(rec, f.off, text_of)
    return {"acm_gpu_scan_anchored_device": [sc.rec_rows(r), sc.i32(tid), sc.i64(first), np.array([r.size])],
            "acm_gpu_lookup_device": [sc.i32(whole), sc.i32(prefix), sc.i32(length)]}


def expected(f, name, which="real"):
    """what entry point `name` must give on the Features' batch, without a device (None: the two of sc.PLAIN_BY_PLAN, whose
    case computes its expected value with the plan's wire bits)"""
    if name in sc.FEATURES:
        return f.expected(name, which)
    if name in sc.ANCHORED:
        return anchored_expected(f, which)[name]
    if name in fc.ENTRIES:
        return fc.expected(f, name, which)
    assert name in sc.PLAIN, name
    return None if name in sc.PLAIN_BY_PLAN else sc.plain_expected(f.o, f.real, f.decoy, which)[name]


def case(torch, f, name):
    """the Case of any of ENTRIES on the plan of `f`, with its expected value in case.want"""
    if name in sc.PLAIN:
        if not hasattr(f, "plain"):
            f.plain = {c.name: c for c in sc.plain_cases(torch, f.plan, f.o, f.real, f.decoy)}
        return f.plain[name]
    if name in sc.ANCHORED:
        c = {c.name: c for c in sc.anchored_cases(torch, f.plan, f.real, f.decoy, f.off)}[name]
        c.want = anchored_expected(f, "real")[name]
        return c
    if name in fc.ENTRIES:
        return fc.case(torch, f, name)
    return f.case(name)
