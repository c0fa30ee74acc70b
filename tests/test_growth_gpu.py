"""Every device entry point behind every way a plan can grow (tests/growth_cases.py: built, born empty, stepwise,
outgrown, merged, a 4-gram base with the sets' pieces as its delta).  Per shape one stream_cases.Features, made once;
per entry point the raw C-ABI call of tests/stream_cases.py and tests/family_stream_cases.py on the null stream: on the
real inputs, on the decoy, on the real inputs again.  Both real answers equal the expected value exactly, order
included -- the oracle's records and the families' definitions in plain Python, never the library's own scan, join or
host pass -- and the decoy's answer is the decoy's expected value; acm_gpu_plan_status is clean behind each.
tests/test_growth_cpu.py holds the sweep against the headers and shows that no shape can pass trivially."""
import numpy as np
import pytest

from tests import family_stream_cases as fc
from tests import growth_cases as gc
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu

_features = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    yield torch
    _features.clear()


def _shape(torch, shape):
    if shape not in _features:
        _features[shape] = gc.features(torch, shape)
    return _features[shape]


def _held(name, what, got, want):
    assert len(got) == len(want), (name, what, len(got), len(want))
    for i, w in enumerate(want):
        assert w is None or sc.same([got[i]], [w]), (name, what, "output %d" % i, sc.show([got[i]]), sc.show([w]))


@pytest.mark.parametrize("entry", gc.ENTRIES)
@pytest.mark.parametrize("shape", gc.SHAPES)
def test_entry_point_on_a_grown_plan(torch_cuda, monkeypatch, shape, entry):
    f = _shape(torch_cuda, shape)
    info = f.plan.info
    if shape in ("born_empty", "stepwise"):
        assert info.delta_keywords == f.K and info.merges == 0
    elif shape == "outgrown":
        assert info.delta_keywords == f.K - 1 and info.merges == 0
    elif shape == "merged":
        assert info.delta_keywords == 0 and info.merges == 1
    elif shape == "gram_base":
        assert info.delta_keywords == f.K - f.base_keywords and info.merges == 0 and info.kernel == 5
    if entry in fc.INDEX:                                # (both forms of the index: tests/test_index_streams_gpu.py)
        monkeypatch.setenv("ACM_GPU_INDEX_LIST", str(fc.index_longest(f)))
    case = gc.case(torch_cuda, f, entry)
    assert case.want is not None and case.want[0] is not None and np.asarray(case.want[0]).size > 0, entry
    run = sc.Run(torch_cuda, None, case)
    first, _ = run.plain("real")
    f.plan.status()
    decoy, _ = run.plain("decoy")
    f.plan.status()
    again, _ = run.plain("real")
    f.plan.status()
    _held(entry, "first call", first, case.want)
    _held(entry, "call behind the decoy's", again, case.want)
    assert not sc.same(decoy, first), (entry, "the decoy gives the real answer")
    other = gc.expected(f, entry, "decoy")
    if other is not None:
        _held(entry, "decoy", decoy, other)


# ---------------------------------------------------------------------------------------------- other symbol sizes, class plans
# The fixed cases of the feature tests, whose bodies take a plan, on plans that grew: start-parallel plans of 2- and
# 4-byte symbols edited in place (once: the tables move out of the creation blob; twice, with a scan between: the patch
# path), an 8-byte plan whose delta interns symbols the base lacks, a class plan whose delta brings class members the
# base never saw.  The expected values are those tests' own: the oracle's records and the definitions.
WIDE = [(sb, how) for sb in (2, 4, 8) for how in gc.HOWS[sb]]


def _probe(torch, text):
    def probe(plan):
        assert int(plan.count(torch.from_numpy(text.view({2: np.int16, 4: np.int32, 8: np.int64}[text.itemsize])).cuda()).item()) >= 0
        plan.status()
    return probe


@pytest.mark.parametrize("sb,how", WIDE)
def test_near_fixed_case_on_a_grown_plan(torch_cuda, sb, how):
    from tests import test_near_gpu as t
    from tests.near_cases import CASE_GROUPS, CASE_KEYWORDS, CASE_TEXT, near, oracle_records
    rec = oracle_records(CASE_KEYWORDS, CASE_TEXT)
    want = near(rec, CASE_GROUPS, len(CASE_TEXT))
    g = gc.grown([t._sym(w, sb) for w in CASE_KEYWORDS], how, sb, probe=_probe(torch_cuda, t._sym(CASE_TEXT, sb)))
    t.fixed_case_on_plan(torch_cuda, g.plan, sb, rec, want)


@pytest.mark.parametrize("sb,how", WIDE)
def test_words_fused_calls_on_a_grown_plan(torch_cuda, novel_bytes, sb, how):
    from tests import test_words_gpu as t
    from tests.words_cases import novel_case
    keywords, text, rec, want = novel_case(novel_bytes)
    g = gc.grown([t._sym(w, sb) for w in keywords], how, sb, probe=_probe(torch_cuda, t._sym(text, sb)))
    t.fused_calls_on_plan(torch_cuda, g.plan, sb, text, rec, want)


@pytest.mark.parametrize("sb,how", WIDE)
def test_grep_gather_on_a_grown_plan(torch_cuda, monkeypatch, kat, sb, how):
    from tests import test_grep_gpu as t
    o, _, base, off = t._alignment_case(sb, monkeypatch, kat, small=True)
    g = gc.grown(t.small_dictionary(sb)[0], how, sb, probe=_probe(torch_cuda, base))
    t.gather_alignment_on_plan(torch_cuda, g.plan, o, base, off, sb)


def _wide_flow_case(sb):
    from tests import flow_cases as fl
    from oracle import pyoracle as po
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[sb]
    o = po.Oracle(sb)
    kws = [np.frombuffer(w, np.uint8).astype(dt) for w in fl.KEYWORDS]
    for w in kws:
        o.add_keyword(w)
    steps = fl.boundary_steps()
    want = fl.expected(o, steps, dt)
    fl.nontrivial(o, steps, want, dt)
    return kws, steps, want, dt


@pytest.mark.parametrize("sb,how", WIDE)
def test_flows_boundary_set_on_a_grown_plan(torch_cuda, sb, how):
    from tests import flow_cases as fl
    from tests.test_flows_gpu import _feed
    kws, steps, want, dt = _wide_flow_case(sb)
    g = gc.grown(kws, how, sb, probe=_probe(torch_cuda, steps[1].buffer(dt)))
    _feed(torch_cuda, g.plan, fl.N_FLOWS, steps, want, dt, what="%d %s" % (sb, how))
    g.plan.status()


@pytest.mark.parametrize("sb,how", WIDE)
def test_plain_scans_on_a_grown_plan(torch_cuda, sb, how):
    """the wide small cases of tests/cases.py for 2 and 4 bytes; for 8 bytes a dictionary over 40 symbols of 64 bits"""
    from oracle import pyoracle as po
    from tests.cases import small_cases
    from tests.test_gpu_parity import bit_exact_on_plan
    if sb == 8:
        rng = np.random.default_rng(88)
        vocab = rng.integers(0, 1 << 63, size=40, dtype=np.uint64)
        kws = [vocab[rng.integers(0, vocab.size, size=rng.integers(1, 5))] for _ in range(120)]
        text = vocab[rng.integers(0, vocab.size, size=30000)]
        text[rng.integers(0, text.size, size=3000)] = rng.integers(0, 1 << 63, size=3000, dtype=np.uint64)      # symbols no keyword has
    else:
        kws, text, _ = small_cases()["u16_symbols" if sb == 2 else "u32_symbols"]
    o = po.Oracle(sb)
    for w in kws:
        o.add_keyword(w)
    assert o.scan(text).size >= 30
    # (two equal keywords are one id: the plan grows by the machine's keywords, first spelling first)
    m = gc.shadow_of(kws, [range(len(kws))], sb)
    g = gc.grown(gc.keywords_of(m), how, sb, probe=_probe(torch_cuda, text))
    assert o.nb_keywords == m.nb_keywords
    bit_exact_on_plan(torch_cuda, g.plan, o, text)


def _class_machine(kat):
    import ctypes as C
    import aho_corasick_1975_amd as acm
    cmp = C.cast(kat.kat_casecmp8, C.c_void_p)

    def new_machine():
        m = acm.Machine(1, cmp=cmp)
        m.set_symbol_bytes(1)
        return m
    return cmp, new_machine


def test_class_plan_outgrown_near_and_plain_scans(torch_cuda, kat):
    """kat_casecmp8's classes: the base plan knows the letters of `he` alone, the delta brings every other class"""
    from tests import test_near_gpu as t
    from tests.near_cases import CASE_KEYWORDS
    from tests.test_gpu_parity import bit_exact_on_plan
    from oracle import pyoracle as po
    cmp, text, rec, want = t.class_case(kat)
    _, new_machine = _class_machine(kat)
    kws = [np.frombuffer(w, np.uint8) for w in CASE_KEYWORDS]
    g = gc.grown(kws, "outgrown", 1, new_machine=new_machine, plan_of=lambda m, device: m.plan_classes(device))
    assert g.plan.info.kernel == 1, g.plan.describe()
    t.class_case_on_plan(torch_cuda, g.plan, text, rec, want)
    o = po.Oracle(1, po.MEYER85, cmp=cmp)
    for w in CASE_KEYWORDS:
        o.add_keyword(w)
    bit_exact_on_plan(torch_cuda, g.plan, o, np.frombuffer(text * 40, np.uint8))


def test_class_plan_outgrown_flows(torch_cuda, kat):
    """the boundary set of the flow tests in mixed case on a class plan whose delta holds all but `he`"""
    from tests import flow_cases as fl
    from tests.test_flows_gpu import _feed
    from oracle import pyoracle as po
    cmp, new_machine = _class_machine(kat)
    o = po.Oracle(1, po.MEYER85, cmp=cmp)
    for w in fl.KEYWORDS:
        o.add_keyword(w)

    def mixed(t):
        a = np.array(t, np.uint8)
        up = (np.arange(a.size) % 3 == 1) & (a >= 97) & (a <= 122)
        a[up] -= 32
        return a
    steps = [fl.Call([mixed(t) for t in s.texts], s.flows) for s in fl.boundary_steps()]
    want = fl.expected(o, steps)
    fl.nontrivial(o, steps, want)
    lower = po.Oracle(1)
    for w in fl.KEYWORDS:
        lower.add_keyword(w)
    assert sum(w[0].size for w in fl.expected(lower, steps)) < sum(w[0].size for w in want)      # (the exact-case reading finds fewer)
    g = gc.grown([np.frombuffer(w, np.uint8) for w in fl.KEYWORDS], "outgrown", 1, new_machine=new_machine,
                 plan_of=lambda m, device: m.plan_classes(device))
    _feed(torch_cuda, g.plan, fl.N_FLOWS, steps, want, what="classes outgrown")
    g.plan.status()


def _class_oracle(cmp, keywords):
    from oracle import pyoracle as po
    o, exact = po.Oracle(1, po.MEYER85, cmp=cmp), po.Oracle(1, po.MEYER85)
    for w in keywords:
        o.add_keyword(w)
        exact.add_keyword(w)
    return o, exact


def test_class_plan_outgrown_words(torch_cuda, kat, novel_bytes):
    """the fused whole-word calls over the novel's opening behind a line in mixed case: the records are the comparator
    oracle's, the word test is on the caller's own symbols; the base plan is `he` alone"""
    from tests import test_words_gpu as t
    from tests.words_cases import NOVEL_KEYWORDS, as_set, words
    cmp, new_machine = _class_machine(kat)
    o, exact = _class_oracle(cmp, NOVEL_KEYWORDS)
    text = b"THE he SHE she hErs hersX Xhers xhers MRS mrs. " + novel_bytes[:6000]
    rec = o.scan(text)
    want = words(rec, text)
    assert exact.scan(text).size < rec.size and 0 < want.size < rec.size and len(as_set(want)) == want.size
    assert np.count_nonzero(want["keyword_id"] > 0) > 0                       # whole words of the delta's keywords
    g = gc.grown([np.frombuffer(w, np.uint8) for w in NOVEL_KEYWORDS], "outgrown", 1, new_machine=new_machine,
                 plan_of=lambda m, device: m.plan_classes(device))
    t.fused_calls_on_plan(torch_cuda, g.plan, 1, text, rec, want)


def test_class_plan_outgrown_grep_gather(torch_cuda, monkeypatch, kat):
    """the gather-alignment batch of the grep tests with every third symbol in upper case; hits by the comparator oracle;
    the base plan is the first keyword alone"""
    from tests import test_grep_gpu as t
    from tests.grep_cases import oracle_hits
    cmp, new_machine = _class_machine(kat)
    kws = t.small_dictionary(1)[0]
    _, _, base, off = t._alignment_case(1, monkeypatch, kat, small=True)
    base = base.copy()
    base[1::3] -= 32
    o, exact = _class_oracle(cmp, kws)
    assert int(oracle_hits(exact, base, off).sum()) < int(oracle_hits(o, base, off).sum())      # (the exact-case reading finds fewer)
    g = gc.grown(kws, "outgrown", 1, new_machine=new_machine, plan_of=lambda m, device: m.plan_classes(device))
    t.gather_alignment_on_plan(torch_cuda, g.plan, o, base, off, 1)
