"""Every device entry point on a stream that is not the default one (include/acm_gpu.h: "The call only queues launches
on `stream`, with no host round trip").  In every other GPU test the stream is the legacy null stream, on which
everything serialises: a kernel, a memset, a hipCUB scan or a copy queued inside an entry point on stream 0 instead of
`stream` gives the right answer there and a race for a caller on a side stream.

tests/stream_cases.py has the mechanism: real and decoy inputs, a gate (torch.cuda._sleep, calibrated once per
module) on one of two streams that do not wait for each other, the other left idle.  EARLY -- gate, copy of the real
inputs and the call on the side stream over zeroed scratch: what runs on stream 0 runs during the gate on the decoy;
LATE -- the gate on the null stream, scratch as a decoy call left it: what runs on stream 0 sits behind the gate and the
stages behind it read what the decoy left; both also assert that the call came back while the gate was still running.
CONTROL -- EARLY with the call on the null stream must give the decoy's answer: the gate is long enough, the streams are
independent.  The expected value is the plain call's on the null stream, and that call is held against the case's own
expected value first (Case.want): the oracle's records and the families' definitions in plain Python
(stream_cases.Features.expected), for every output that has a definition -- never the library's own scan, join or host pass.

The gate is 100 ms, or 50 times the plain call's wall time where that is more (never seen: on an MI355X the longest
plain call of this module, synchronise included, took 0.56 ms, and _sleep ran at 2.40 million cycles per millisecond)."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from tests import anchored_cases as ac
from tests import stream_cases as sc
from tests.cases import build_pair
from tests.tally_cases import KINDS, kind, planted
from tests.test_scratch_bounds_gpu import KEYWORDS, _batch

N_PLAIN = 1 << 16                                        # symbols of the plain scans: the text of a plan kind cut to its first 64 Ki


# ---------------------------------------------------------------------------------------------- the completeness guard (no GPU)
def test_every_stream_entry_point_has_a_case():
    """a function of include/acm_gpu.h with a `void *stream` parameter is in the table of cases or excluded with a reason"""
    declared = sc.header_stream_functions()
    assert len(declared) >= 40 and len(set(declared)) == len(declared), declared
    assert len(set(sc.CASES)) == len(sc.CASES) and not set(sc.CASES) & set(sc.EXCLUDED)
    missing = [f for f in declared if f not in sc.CASES and f not in sc.EXCLUDED]
    assert not missing, "no stream case for %s" % missing
    stale = [f for f in list(sc.CASES) + list(sc.EXCLUDED) if f not in declared]
    assert not stale, "not declared with a stream any more: %s" % stale
    assert all(isinstance(r, str) and len(r) > 20 for r in sc.EXCLUDED.values())
    for f in sc.FEATURES:                                # every feature entry point of the table has its builder
        assert hasattr(sc.Features, "_" + f[len("acm_gpu_"):]), f
    assert set(sc.CONTROLS) <= set(sc.CASES) and set(sc.FUSED) <= set(sc.FEATURES)


# ---------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def gates(torch_cuda):
    g = sc.Gates(torch_cuda)
    yield g
    torch_cuda.cuda.synchronize()
    print("gates: %.0f cycles per ms, longest plain call %.3f ms, longest gate %.0f ms" % (g.cycles_per_ms, g.longest_plain_ms, g.longest_gate_ms))


def _decoy_batch():
    """a second text over _batch ()'s alphabet, for the same offsets"""
    rng = np.random.default_rng(76)
    return np.frombuffer(b"hesir .", np.uint8)[rng.integers(0, 7, size=4096)].copy()


@pytest.fixture(scope="module")
def dense_features(torch_cuda):
    text, off = _batch()
    m, o = build_pair(KEYWORDS, 1)
    f = sc.Features(torch_cuda, m, o, m.plan, text, _decoy_batch(), off)
    assert f.plan.info.kernel == 1, f.plan.describe()
    return f


@pytest.fixture(scope="module")
def gram_features(torch_cuda):
    """the 4-gram kind of tests/tally_cases.py over _batch ()'s offsets: two stretches of its text with keywords planted,
    words cut at n to z"""
    _, off = _batch()
    m, o, text, make_plan, plan_ok, _ = kind("gram", None, None)
    f = sc.Features(torch_cuda, m, o, make_plan, planted(text[:4096], 77), planted(text[8192:12288], 78), off, word_ranges=((0x61, 0x6D),))
    assert plan_ok(f.plan), f.plan.describe()
    return f


def _pass(bad):
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- the plain scans, per plan kind
def _plain_texts(name, text, novel_bytes=None):
    """the kind's text cut to its first 64 Ki symbols; as the decoy the same symbols rotated by 12,345 places, with 500
    symbols of every 4,096 overwritten by one symbol: other positions and another count, whichever stretch holds the matches"""
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    at = 1 if name == "csr" else 0                       # (the CSR walk is what a dense plan launches on a text off the 16-byte grid)
    real = text[at:at + N_PLAIN].copy()
    assert real.size == N_PLAIN
    decoy = np.roll(real, 12345)
    for b in range(0, N_PLAIN, 4096):
        decoy[b + 100:b + 600] = real[0]
    return real, decoy


def _plain(torch_cuda, gates, name, monkeypatch, kat, novel_bytes):
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    real, decoy = _plain_texts(name, text, novel_bytes)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    bad = []
    for case in sc.plain_cases(torch_cuda, plan, o, real, decoy, misalign=name == "csr"):
        bad += sc.exercise(torch_cuda, gates, case, control=case.name in ("acm_gpu_scan_device", "acm_gpu_scan_ordered_device"))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", KINDS)
def test_plain_scans_every_plan_kind(torch_cuda, gates, monkeypatch, kat, novel_bytes, name):
    """scan, count, ordered scan, bucket order, radix sort, pack and unpack on dense, 4-gram, CSR, start-parallel, sparse
    walk, 8-byte, class and delta plans: early and late, the two scans with a control"""
    _pass(_plain(torch_cuda, gates, name, monkeypatch, kat, novel_bytes))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dense", "gram"])
def test_plain_scans_in_launch_segments(torch_cuda, gates, monkeypatch, kat, novel_bytes, name):
    """ACM_GPU_SEGMENT_LOG2=13: eight launch segments per call"""
    monkeypatch.setenv("ACM_GPU_SEGMENT_LOG2", "13")
    _pass(_plain(torch_cuda, gates, name, monkeypatch, kat, novel_bytes))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["starts", "dense"])
def test_update_in_front_of_the_first_scan_on_the_side_stream(torch_cuda, gates, monkeypatch, kat, name):
    """acm_gpu_plan_update, then the first scan on the side stream: a start-parallel plan's new state words "are written
    on the stream of the next scan, in front of it", every other plan scans its new delta plan behind its own.  The
    expected value is the oracle's with the new keyword.  The answers are held in both arrangements; that the call only
    queues work is held wherever the header says so (not for the scan behind a start-parallel plan's first update)."""
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    real, decoy = _plain_texts(name, text)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    scan = sc.plain_cases(torch_cuda, plan, o, real, decoy)[0]    # (no scratch whose size an update could change)
    assert scan.name == "acm_gpu_scan_device"
    run = sc.Run(torch_cuda, gates, scan)
    want, _ = run.plain("real")
    _, plain_ms = run.plain("decoy")
    gate_ms = gates.length_ms(plain_ms)
    bad = []
    for arrangement, at in (("early", 1000), ("late", 3000)):
        new = real[at:at + 5].copy()                     # five symbols of the real text: a keyword that occurs
        before = o.scan(real).size
        m.add_keyword(new)
        o.add_keyword(new)
        expected = o.scan(real)
        assert before < expected.size <= scan.outs["rec"][0] // 2, (before, expected.size)
        plan.update(m)
        got, ok = run.early(gate_ms) if arrangement == "early" else run.late(gate_ms)
        if not sc.same(got, [sc.sorted_rows(sc.rec_rows(expected)), np.array([expected.size])]):
            bad.append("%s %s behind an update: %s, want %d records" % (name, arrangement, sc.show(got), expected.size))
        # include/acm_gpu.h, acm_gpu_plan_update: the scan behind an update of a start-parallel plan "is the one call of such a
        # plan that is NOT only queued"; "the first update of a plan [...] waits for the whole device".  The late arrangement's
        # is the second update: its copy waits for the side stream alone, which the null stream's gate does not hold up.
        if not ok and not (name == "starts" and arrangement == "early"):
            bad.append("%s %s behind an update: the call waited" % (name, arrangement))
        run.plain("decoy")
    _pass(bad)


# ---------------------------------------------------------------------------------------------- every other entry point
@pytest.mark.gpu
@pytest.mark.parametrize("entry", sc.FEATURES)
def test_feature_entry_points_dense(torch_cuda, gates, dense_features, entry):
    """{he, she, his, hers} and the pieces of the set families, 4 Ki symbols in 37 texts"""
    _pass(sc.exercise(torch_cuda, gates, dense_features.case(entry), control=entry in sc.CONTROLS))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sc.FUSED)
def test_fused_entry_points_gram(torch_cuda, gates, gram_features, entry):
    """the fused forms once more where the scan writes its records itself and the ordered scan is the tiled pass"""
    _pass(sc.exercise(torch_cuda, gates, gram_features.case(entry)))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sc.ANCHORED)
def test_anchored_entry_points(torch_cuda, gates, entry):
    """the anchored tests' hand-made batch; the decoy is the same buffer read backwards"""
    m, o = build_pair(ac.KEYWORDS, 1)
    real = np.frombuffer(b"".join(ac.TEXTS), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(t) for t in ac.TEXTS])]).astype(np.uint64)
    decoy = real[::-1].copy()
    want, look = [], []
    for text in (real, decoy):                           # on the CPU, by the oracle and the definitions
        rec, text_of = ac.batch_records(o, text, off)
        want.append(ac.anchored(rec, off, ac.PREFIXES, text_of))
        look.append(ac.lookup(rec, off, text_of))
    assert want[0][0].size == ac.N_PREFIXES and 0 < want[1][0].size != want[0][0].size
    assert not all(np.array_equal(a, b) for a, b in zip(look[0], look[1]))
    case = {c.name: c for c in sc.anchored_cases(torch_cuda, m.plan(0), real, decoy, off)}[entry]
    if entry == "acm_gpu_scan_anchored_device":
        r, tid, first = want[0]
        case.want = [sc.rec_rows(r), sc.i32(tid), sc.i64(first), np.array([r.size])]
    else:
        case.want = [sc.i32(a) for a in look[0]]
    _pass(sc.exercise(torch_cuda, gates, case, control=entry in sc.CONTROLS))


@pytest.mark.gpu
def test_synth_text(torch_cuda, gates):
    """the bench's device text generator takes a stream as well"""
    kd, ko = acm.synth.keywords(200)
    m, _ = build_pair([b"he"], 1)
    case = sc.synth_case(torch_cuda, m.plan(0), kd, ko)
    case.want = [acm.synth.text(1 << 16, kd, ko)]
    _pass(sc.exercise(torch_cuda, gates, case, control=True))
