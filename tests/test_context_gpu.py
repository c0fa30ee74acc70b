"""Match contexts on the GPU (acm_gpu_context_*, acm_gpu_scan_context_*, acm_context;
csrc/dev_context.h).  The expected answer is always the definition of CONTEXT in plain Python over the
ORACLE's records or over hand-made records (tests/context_cases.py: the window formula for EACH, a cover
array for MERGE), never the library's own scan or passes.  Texts are a few KiB and hold a few thousand
records; one case has more record tiles than the capped grid has blocks, so that blocks stride over tiles."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import broken_last_pair
from tests.cases import build_pair
from tests.context_cases import BATCH_TEXTS, KEYWORDS, MOST, NONE, Expected, batch_case, expected, line_offsets, not_vacuous, novel_page, oracle_records
from tests.tally_cases import PATH_CLASSES, PATH_GPU, kind

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a copy of the low byte alone is seen
GUARD = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _dev(torch, arr):
    a = np.frombuffer(bytes(arr), dtype=np.uint8) if isinstance(arr, (bytes, bytearray)) else np.ascontiguousarray(arr)
    a = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])
    return torch.from_numpy(a.copy()).cuda()


def _rec_dev(torch, rec, room=None):
    a = np.zeros(max(rec.size if room is None else room, 1), po.RECORD_DTYPE)
    a[:rec.size] = rec
    return torch.from_numpy(a.view(np.int64).reshape(-1, 2).copy()).cuda()


def _rec_host(t, n):
    return np.frombuffer(t[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()


def _sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(DTYPE[sb])


def _np(t, dtype, n):
    return t[:n].cpu().numpy().view(dtype)


def _check(s, exp, text, m, what=None):
    """a Snippets of device tensors against the expectation, array by array; `text` is the symbols as a numpy array, m the records"""
    assert (s.n_snippets, s.out_symbols) == (exp.n_snippets, exp.out_symbols), (what, s.n_snippets, s.out_symbols, exp.n_snippets, exp.out_symbols)
    k = exp.n_snippets
    assert np.array_equal(_np(s.snip_lo, np.uint64, k), exp.snip_lo), what
    assert np.array_equal(_np(s.out_offsets, np.uint64, k + 1), exp.out_offsets), what
    assert np.array_equal(_np(s.snip_text, np.uint32, k), exp.snip_text), (what, _np(s.snip_text, np.uint32, k), exp.snip_text)
    assert np.array_equal(_np(s.rec_snip, np.uint32, m), exp.rec_snip), what
    assert np.array_equal(_np(s.rec_at, np.int64, m), exp.rec_at), what
    if s.out is not None and exp.out_symbols <= s.out_capacity:
        want = exp.out(text)
        got = s.out[:want.size * want.itemsize].cpu().numpy().view(want.dtype)
        assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
        if k:
            assert np.array_equal(s[k - 1].cpu().numpy().view(want.dtype), want[int(exp.out_offsets[k - 1]):])


def _guarded(torch, sb, room, k):
    """(whole, out): a uint8 tensor filled with GUARD and the view of `room` symbols that begins k symbols behind its
    16-byte aligned front"""
    whole = torch.full(((k + room) * sb + 64,), GUARD, dtype=torch.uint8, device="cuda")
    out = whole[k * sb:(k + room) * sb]
    assert whole.data_ptr() % 16 == 0 and out.data_ptr() % 16 == k * sb % 16
    return whole, out


def _guards_hold(whole, sb, k, used):
    """nothing but out[0 .. used) symbols was written"""
    h = whole.cpu().numpy()
    return (h[:k * sb] == GUARD).all() and (h[(k + used) * sb:] == GUARD).all()


def cover_expected(s, e, n, before, after):
    """MERGE | SYMBOLS over ONE text for records with starts s and ends e (numpy, ascending ends): the cover array
    without a Python loop over the buffer"""
    lo = np.maximum(s - np.minimum(before, s), 0)
    hi = np.minimum(e + 1 + after, n)
    d = np.zeros(n + 1, np.int64)
    np.add.at(d, lo, 1)
    np.add.at(d, hi, -1)
    cover = np.concatenate([[False], np.cumsum(d)[:n] > 0, [False]])
    begins = np.flatnonzero(cover[1:-1] & ~cover[:-2])
    ends = np.flatnonzero(cover[1:-1] & ~cover[2:]) + 1
    lens = ends - begins
    at = np.concatenate([[0], np.cumsum(lens)])
    q = np.searchsorted(begins, s, "right") - 1
    return Expected(begins, lens, np.zeros(begins.size, np.uint32), q, at[q] + s - begins[q])


_plans = {}


def _plan(sb, monkeypatch, kat):
    """a plan of the symbol size, made once (tests/test_words_gpu.py's choice): the context passes use a plan for its
    device, its symbol size and its grid cap only"""
    if sb not in _plans:
        if sb == 2:
            m, o = build_pair([np.array([104, 101], np.uint16), np.array([115], np.uint16)], 2)
            _plans[sb] = (m, m.plan(0))
        else:
            m, o, text, make_plan, plan_ok, form = kind({1: "dense", 4: "starts", 8: "u64"}[sb], monkeypatch, kat)
            plan = make_plan(0)
            assert plan_ok(plan) and plan.sym_size == sb
            _plans[sb] = (m, plan)
    return _plans[sb][1]


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_every_symbol_size_alignment_and_window(torch_cuda, monkeypatch, kat, novel_bytes, sb):
    """a match at symbol 0 and one that ends at n - 1; d_text and d_out at an aligned allocation and one symbol past
    it; an output tile of 256 bytes, so that snippets straddle tiles and 16-byte words; guards round d_out"""
    torch = torch_cuda
    monkeypatch.setenv("ACM_GPU_CONTEXT_OUT_TILE", "256")
    plan = _plan(sb, monkeypatch, kat)
    text = b"he" + novel_bytes[200:1500] + b" hers she"
    n = len(text)
    rec = oracle_records(KEYWORDS, text)
    assert int(rec["end_pos"][0]) == 1 and int(rec["end_pos"][-1]) == n - 1 and rec.size > 30
    sym = _sym(text, sb)
    d_rec = _rec_dev(torch, rec)
    for k_text in (16 // sb, 1):
        whole_text = _dev(torch, np.concatenate([np.repeat(_sym(b"#", sb), k_text), sym, np.repeat(_sym(b"#", sb), 16)]))
        dev = whole_text[k_text:k_text + n]
        assert whole_text.data_ptr() % 16 == 0 and dev.data_ptr() % 16 == k_text * sb % 16
        for k_out in (0, 1):
            for before, after in ((0, 0), (3, 5), (40, 40), (MOST, MOST)):
                for merged in (True, False):
                    exp = expected(rec, n, None, before, after, merged=merged)
                    if merged and before != MOST:
                        not_vacuous(exp, rec.size)
                    whole, out = _guarded(torch, sb, exp.out_symbols, k_out)
                    s = plan.context_records(dev, d_rec, rec.size, before=before, after=after, merge=merged, out=out)
                    _check(s, exp, sym, rec.size, (sb, k_text, k_out, before, after, merged))
                    assert _guards_hold(whole, sb, k_out, exp.out_symbols), (sb, k_text, k_out, before, after, merged)
    assert expected(rec, n, None, MOST, MOST).out_symbols == n
    plan.status()


def test_nested_and_touching_windows_without_context(torch_cuda):
    """before = after = 0: `he` inside `she` merges with it, and "hehe" touches and is one snippet"""
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    text = b"she hehe x he"
    rec = oracle_records(KEYWORDS, text)
    exp = not_vacuous(expected(rec, len(text)), rec.size)
    assert [(int(a), int(n)) for a, n in zip(exp.snip_lo, exp.lens)] == [(0, 3), (4, 4), (11, 2)]
    s = plan.context_records(_dev(torch_cuda, text), _rec_dev(torch_cuda, rec), rec.size)
    _check(s, exp, np.frombuffer(text, np.uint8), rec.size)
    assert bytes(s[1].cpu().numpy()) == b"hehe"
    plan.status()


def test_a_snippet_over_several_record_tiles(torch_cuda, monkeypatch):
    """tiles of 64 records, keyword `a` over 300 `a`s: one snippet spans five record tiles, so the suffix minimum and
    the snippet's number are carried across several tiles; with before = 70 the first record of the NEXT run reaches
    back over a whole tile of the run in front"""
    monkeypatch.setenv("ACM_GPU_CONTEXT_TILE", "64")
    m, o = build_pair([b"a"], 1)
    plan = m.plan(0)
    text = b"a" * 300 + b"b" * 90 + b"a" * 200 + b"b" * 60 + b"a"
    rec = oracle_records([b"a"], text)
    t = np.frombuffer(text, np.uint8)
    dev, d_rec = _dev(torch_cuda, text), _rec_dev(torch_cuda, rec)
    for before, after, snippets in ((0, 0, 3), (70, 0, 2), (0, 70, 2), (5, 5, 3), (100, 100, 1)):
        exp = expected(rec, len(text), None, before, after)
        assert exp.n_snippets == snippets and (snippets == 1 or 1 < exp.n_snippets < rec.size)
        _check(plan.context_records(dev, d_rec, rec.size, before=before, after=after), exp, t, rec.size, (before, after))
        _check(plan.context_records(dev, d_rec, rec.size, before=before, after=after, merge=False),
               expected(rec, len(text), None, before, after, merged=False), t, rec.size, (before, after, "each"))
    plan.status()


def test_more_record_tiles_than_the_grid_has_blocks(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles"""
    monkeypatch.setenv("ACM_GPU_CONTEXT_TILE", "64")
    m, o = build_pair([b"a"], 1)
    plan = m.plan(0)
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n_rec = (8 * cus + 3) * 64 + 65
    rng = np.random.default_rng(11)
    gaps = rng.choice(np.array([1, 1, 1, 2, 3, 9, 40]), size=n_rec)          # the `a`s lie 1 .. 40 symbols apart
    pos = np.cumsum(gaps) - 1
    n = int(pos[-1]) + 1
    t = np.full(n, ord("b"), np.uint8)
    t[pos] = ord("a")
    rec = np.zeros(n_rec, po.RECORD_DTYPE)
    rec["end_pos"], rec["length"] = pos, 1
    assert np.array_equal(oracle_records([b"a"], t[:3000].tobytes()), rec[:np.searchsorted(pos, 3000)])
    dev, d_rec = _dev(torch_cuda, t), _rec_dev(torch_cuda, rec)
    for before, after in ((0, 0), (2, 1), (12, 0)):
        exp = not_vacuous(cover_expected(pos, pos, n, before, after), n_rec)
        small = expected(rec[:400], int(pos[399]) + 1, None, before, after)       # (the loop agrees where it is affordable)
        assert np.array_equal(small.snip_lo[:-1], exp.snip_lo[:small.n_snippets - 1]) and np.array_equal(small.rec_at[:300], exp.rec_at[:300])
        _check(plan.context_records(dev, d_rec, n_rec, before=before, after=after), exp, t, n_rec, (before, after))
    plan.status()


def test_a_batch_with_every_boundary_case(torch_cuda, monkeypatch):
    """windows clipped at their text's two ends, two windows that touch across a boundary (two snippets under SYMBOLS,
    one under TEXTS), empty texts, windowless records from the ordered scan of the packed buffer, TEXTS reaching past
    the first and the last text -- repeated until the records fill several tiles of 64"""
    monkeypatch.setenv("ACM_GPU_CONTEXT_TILE", "64")
    monkeypatch.setenv("ACM_GPU_CONTEXT_OUT_TILE", "256")
    texts = BATCH_TEXTS * 12
    packed = b"".join(texts)
    off = np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.uint64)
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    rec = oracle_records(KEYWORDS, packed)
    t = np.frombuffer(packed, np.uint8)
    dev, d_off = _dev(torch_cuda, packed), _dev(torch_cuda, off.astype(np.int64))
    # the ordered scan of the packed buffer is what goes in, records across the cuts included
    scanned = plan.scan_context(dev, d_off, before=2, after=3, capacity=rec.size)
    assert scanned.count == rec.size and np.array_equal(_rec_host(scanned.records, rec.size), rec)
    d_rec = scanned.records
    one = batch_case()
    sym, tex = expected(one[2], len(one[0]), one[1], 0, 0), expected(one[2], len(one[0]), one[1], 0, 0, texts=True)
    b = int(one[1][BATCH_TEXTS.index(b"he")])
    assert b in sym.snip_lo and b not in tex.snip_lo and NONE in sym.rec_snip                  # touching across a boundary; a windowless record
    for texts_unit, before, after in ((False, 0, 0), (False, 2, 3), (False, MOST, MOST), (True, 0, 0), (True, 1, 1), (True, 0, 2), (True, 300, 300),
                                      (True, MOST, MOST)):
        for merged in (True, False):
            exp = expected(rec, len(packed), off, before, after, texts_unit, merged)
            if merged and before < 300:
                not_vacuous(exp, rec.size)
            s = plan.context_records(dev, d_rec, rec.size, offsets=d_off, before=before, after=after, unit="texts" if texts_unit else "symbols",
                                     merge=merged, out_capacity=exp.out_symbols)
            _check(s, exp, t, rec.size, (texts_unit, before, after, merged))
    _check(scanned, expected(rec, len(packed), off, 2, 3), t, rec.size)
    got = plan.scan_context_host(t, offsets=off, before=1, after=1, unit="texts")
    exp = expected(rec, len(packed), off, 1, 1, texts=True)
    assert np.array_equal(got.out, exp.out(t)) and np.array_equal(got.snip_text, exp.snip_text) and np.array_equal(got.rec_at, exp.rec_at)
    assert np.array_equal(got.records, rec)
    plan.status()                                                                               # a record across a cut is no error


def test_counts_on_the_device_no_records_and_overflows(torch_cuda, novel_bytes):
    torch = torch_cuda
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    text, rec, _ = novel_page(novel_bytes)
    t = np.frombuffer(text, np.uint8)
    dev = _dev(torch, text)
    exp = not_vacuous(expected(rec, len(text), None, 8, 8), rec.size)
    # d_n given: n is the room
    room = rec.size + 100
    d_rec = _rec_dev(torch, rec, room)
    count = torch.tensor([rec.size], dtype=torch.int64, device="cuda")
    _check(plan.context_records(dev, d_rec, room, before=8, after=8, count=count), exp, t, rec.size)
    # no records at all: by a count of 0 on the device, and by no room
    for merged in (True, False):
        whole, out = _guarded(torch, 1, 64, 1)
        s = plan.context_records(dev, d_rec, room, before=8, after=8, merge=merged, count=torch.zeros(1, dtype=torch.int64, device="cuda"), out=out)
        assert (s.n_snippets, s.out_symbols) == (0, 0) and int(s.out_offsets[0].item()) == 0 and _guards_hold(whole, 1, 1, 0)
    s = plan.context_records(dev, d_rec, 0, before=8, after=8)
    assert (s.n_snippets, s.out_symbols) == (0, 0) and int(s.out_offsets[0].item()) == 0
    # *d_n > n_or_capacity: the two counts are 0 and nothing else is written
    L = acm.lib()
    tb = L.acm_gpu_context_tmp_bytes(plan.h, room, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    res = torch.full((2,), 0x5A5A, dtype=torch.int64, device="cuda")
    arrays = [torch.full((room + 1,), 0x5A5A, dtype=torch.int64, device="cuda") for _ in range(5)]
    whole, out = _guarded(torch, 1, len(text), 1)
    over = torch.tensor([room + 1], dtype=torch.int64, device="cuda")

    def call(cnt, cap, flags=2, offsets=None, n_texts=0, records=d_rec):
        return L.acm_gpu_context_records_device(plan.h, dev.data_ptr(), len(text), 0, offsets, n_texts, records.data_ptr(), room, cnt.data_ptr(), 8, 8, flags,
                                                out.data_ptr(), cap, res.data_ptr(), res.data_ptr() + 8, arrays[0].data_ptr(), arrays[1].data_ptr(),
                                                arrays[2].data_ptr(), arrays[3].data_ptr(), arrays[4].data_ptr(), tmp.data_ptr(), tb, None)
    untouched = lambda: all((a.cpu().numpy() == 0x5A5A).all() for a in arrays) and _guards_hold(whole, 1, 1, 0)
    assert call(over, len(text)) == 0
    torch.cuda.synchronize()
    assert res.tolist() == [0, 0] and untouched()
    plan.status()
    # an out_capacity one symbol short: the needed size comes back, the guards are intact, the index arrays are valid
    res.fill_(0x5A5A)
    assert call(count, exp.out_symbols - 1) == 0
    torch.cuda.synchronize()
    assert res.tolist() == [exp.out_symbols, exp.n_snippets] and _guards_hold(whole, 1, 1, 0)
    k = exp.n_snippets
    assert np.array_equal(_np(arrays[0], np.uint64, k), exp.snip_lo) and np.array_equal(_np(arrays[1], np.uint64, k + 1), exp.out_offsets)
    assert np.array_equal(_np(arrays[3].view(torch.int32), np.uint32, rec.size), exp.rec_snip) and np.array_equal(_np(arrays[4], np.int64, rec.size), exp.rec_at)
    plan.status()
    # exactly enough
    assert call(count, exp.out_symbols) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:exp.out_symbols].cpu().numpy(), exp.out(t)) and _guards_hold(whole, 1, 1, exp.out_symbols)
    # the arguments
    assert tb > 0 and L.acm_gpu_context_tmp_bytes(plan.h, 1 << 31, 0) == 0 and L.acm_gpu_scan_context_tmp_bytes(plan.h, 1 << 31, 64, 0) == 0
    for flags in (1, 3, 4, 7):                                                  # TEXTS without offsets, flags above 3
        assert call(count, exp.out_symbols, flags=flags) == E_ARG
    assert L.acm_gpu_context_records_device(plan.h, dev.data_ptr(), len(text), 0, None, 0, d_rec.data_ptr(), room, count.data_ptr(), 8, 8, 2, dev.data_ptr() + 5,
                                            64, res.data_ptr(), res.data_ptr() + 8, arrays[0].data_ptr(), arrays[1].data_ptr(), None, None, None,
                                            tmp.data_ptr(), tb, None) == E_ARG       # d_out inside d_text
    assert L.acm_gpu_context_records_device(plan.h, dev.data_ptr(), len(text), 0, None, 0, d_rec.data_ptr(), room, count.data_ptr(), 8, 8, 2, out.data_ptr(),
                                            64, res.data_ptr(), res.data_ptr() + 8, arrays[0].data_ptr(), arrays[1].data_ptr(), None, None, None,
                                            tmp.data_ptr(), tb - 1, None) == E_ARG   # scratch too small
    plan.status()


def test_contract_violations_report_and_write_nothing(torch_cuda):
    """MERGE over records with a decreasing end_pos, a record out of range and bad offsets: status -7, counts 0, d_out
    and the arrays untouched"""
    torch = torch_cuda
    packed, off, rec = batch_case()
    m, o = build_pair(KEYWORDS, 1)
    dev = _dev(torch, packed)
    n = len(packed)
    swapped = rec.copy()
    swapped[[3, 9]] = swapped[[9, 3]]
    beyond = np.concatenate([rec[:5], np.array([(n, 1, 9)], po.RECORD_DTYPE), rec[5:]])
    long = np.concatenate([rec[:5], np.array([(int(rec["end_pos"][5]), 100, 9)], po.RECORD_DTYPE), rec[5:]])
    cases = [("decreasing end_pos", swapped, off, True), ("beyond the buffer", beyond, off, True), ("beyond, EACH", beyond, off, False),
             ("a start below 0", long, None, True)]
    cases += [(what, rec, np.array(bad, np.uint64), merged) for what, bad in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]),
                                                                              ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n]), *broken_last_pair(n))
              for merged in (True, False)]
    for what, records, offsets, merged in cases:
        plan = m.plan(0)
        plan.status()
        whole, out = _guarded(torch, 1, n, 1)
        s = plan.context_records(dev, _rec_dev(torch, records), records.size, offsets=_dev(torch, offsets.astype(np.int64)) if offsets is not None else None,
                                 before=2, after=3, merge=merged, out=out)
        assert (s.n_snippets, s.out_symbols) == (0, 0), what
        assert _guards_hold(whole, 1, 1, 0), what
        for a in (s.snip_lo, s.out_offsets, s.snip_text, s.rec_snip, s.rec_at):
            assert not a.cpu().numpy().any(), what                             # (the binding hands in zeroed arrays)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()
    # EACH takes the swapped records
    plan = m.plan(0)
    s = plan.context_records(dev, _rec_dev(torch, swapped), swapped.size, offsets=_dev(torch, off.astype(np.int64)), before=2, after=3, merge=False)
    _check(s, expected(swapped, n, off, 2, 3, merged=False), np.frombuffer(packed, np.uint8), swapped.size)
    plan.status()


@pytest.mark.parametrize("name", ["dense", "starts", "u64"])
def test_the_fused_call_on_three_plan_kinds(torch_cuda, monkeypatch, kat, name):
    torch = torch_cuda
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    sb = plan.sym_size
    t = np.ascontiguousarray(text).view(DTYPE[sb])[:20000]
    rec = o.scan(t)
    assert rec.size > 100
    dev = _dev(torch, t)
    for before, after, merged in ((2, 2, True), (0, 0, True), (3, 1, False)):
        exp = expected(rec, t.size, None, before, after, merged=merged)
        if merged:
            not_vacuous(exp, rec.size)
        s = plan.scan_context(dev, before=before, after=after, merge=merged, capacity=rec.size)
        assert s.count == rec.size and np.array_equal(_rec_host(s.records, rec.size), rec)
        _check(s, exp, t, rec.size, (name, before, after, merged))
    # capacity one short of ALL matches: the scan's count, the snippet outputs 0
    s = plan.scan_context(dev, before=2, after=2, capacity=rec.size - 1)
    assert (s.count, s.n_snippets, s.out_symbols) == (rec.size, 0, 0)
    # host memory in, blocking: the two overflows, told apart by *n_found
    exp = expected(rec, t.size, None, 2, 2)
    L = acm.lib()
    nf, ns, sym = C.c_uint64(0), C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    out = np.full(exp.out_symbols, 0, DTYPE[sb])
    lo = np.zeros(rec.size, np.uint64)
    assert L.acm_gpu_scan_context_host(plan.h, t.ctypes.data, t.size, 0, None, 0, None, rec.size - 1, C.byref(nf), 2, 2, 2, out.ctypes.data, out.size,
                                       C.byref(sym), C.byref(ns), lo.ctypes.data, None, None, None, None) == E_OVERFLOW
    assert nf.value == rec.size and ns.value == 0xDEAD
    assert L.acm_gpu_scan_context_host(plan.h, t.ctypes.data, t.size, 0, None, 0, None, rec.size, C.byref(nf), 2, 2, 2, out.ctypes.data, out.size - 1,
                                       C.byref(sym), C.byref(ns), lo.ctypes.data, None, None, None, None) == E_OVERFLOW
    assert (nf.value, ns.value, sym.value) == (rec.size, exp.n_snippets, exp.out_symbols) and np.array_equal(lo[:exp.n_snippets], exp.snip_lo) and not out.any()
    got = plan.scan_context_host(t, before=2, after=2)                                         # the rooms grow once where they must
    assert np.array_equal(got.out, exp.out(t)) and np.array_equal(got.rec_at, exp.rec_at) and np.array_equal(got.records, rec)
    plan.status()


def test_machine_context_on_the_gpu_and_classes_paths(torch_cuda, monkeypatch, kat, novel_bytes):
    text, rec, _ = novel_page(novel_bytes)
    m, o = build_pair(KEYWORDS, 1)
    exp = not_vacuous(expected(rec, len(text), None, 8, 8), rec.size)
    t = np.frombuffer(text, np.uint8)
    s = m.context(t, before=8, after=8)
    assert m.scan_path == PATH_GPU and np.array_equal(s.records, rec)
    assert np.array_equal(s.out, exp.out(t)) and np.array_equal(s.snip_lo, exp.snip_lo) and np.array_equal(s.rec_snip, exp.rec_snip)
    assert np.array_equal(s.rec_at, exp.rec_at) and np.array_equal(s.out_offsets, exp.out_offsets) and bytes(s[3]) == bytes(exp.out(t)[int(exp.out_offsets[3]):int(exp.out_offsets[4])])
    each = m.context(t, before=3, after=5, merge=False)
    assert np.array_equal(each.out, expected(rec, len(text), None, 3, 5, merged=False).out(t))
    with pytest.raises(acm.ACMError) as e:
        m.context(t, before=8, after=8, capacity=rec.size - 1)
    assert e.value.code == E_OVERFLOW
    # a class plan copies the caller's own symbols: upper case stays upper case
    mc, oc, _, make_plan, plan_ok, _ = kind("classes", monkeypatch, kat)
    text = b"THE he SHE she hErs hersX Xhers xhers MRS mrs. " + novel_bytes[:3000]
    rec = oc.scan(text)
    exp = not_vacuous(expected(rec, len(text), None, 4, 4), rec.size)
    t = np.frombuffer(text, np.uint8)
    s = mc.context(t, before=4, after=4)
    assert mc.scan_path == PATH_CLASSES and np.array_equal(s.records, rec)
    assert np.array_equal(s.out, exp.out(t)) and bytes(s[0]).startswith(b"THE he SHE") and np.array_equal(s.rec_at, exp.rec_at)


def test_grep_context_lines(torch_cuda, novel_bytes):
    """Plan.grep_context_lines: split, then TEXTS | MERGE, all on the device -- `grep -F -f keywords -C n file`"""
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    text = novel_bytes[:4096]
    rec = oracle_records(KEYWORDS, text)
    lines = line_offsets(text)
    t = np.frombuffer(text, np.uint8)
    dev = _dev(torch_cuda, text)
    for before, after in ((1, 1), (0, 1), (2, 0), (0, 0)):
        exp = not_vacuous(expected(rec, len(text), lines, before, after, texts=True), rec.size)
        s = plan.grep_context_lines(dev, before=before, after=after, capacity=rec.size)
        assert np.array_equal(s.offsets.cpu().numpy().view(np.uint64), lines)
        _check(s, exp, t, rec.size, (before, after))
        first = int(exp.snip_text[1])
        assert bytes(s[1].cpu().numpy()).startswith(text[int(lines[first]):int(lines[first + 1])])     # snip_text is the group's first line
    plan.status()
