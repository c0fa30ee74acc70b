"""Unordered keyword proximity on the GPU (acm_gpu_near_*, acm_gpu_scan_near_*, acm_scan_near; csrc/dev_near.h).
The expected answer is always the definition of NEAR in plain Python over the ORACLE's records
(tests/near_cases.py: every first symbol tried downwards) and, for byte text, a second derivation from the text
alone -- never the library's own scan or join, and never its closed form.  All comparisons are exact, order
included.  Texts are a few hundred symbols; one case has more records than the capped grid has tiles of 64, so
that blocks stride over tiles, and one has walks of hundreds of records, so that the wave finishes them."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import broken_last_pair
from tests.near_cases import (CASE_CUT, CASE_GROUPS, CASE_KEYWORDS, CASE_TEXT, as_records, case_facts, near, near_by_text, oracle_records, random_cases)
from tests.tally_cases import PATH_CLASSES, PATH_GPU

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
SENTINEL = 0x0123456789ABCDEF
WIDTH_MAX = 1 << 20
BASES = ((1 << 32) - 20, (1 << 63) + 5)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def fixed():
    """(the oracle's records of the fixed case, NEAR of them): computed once, never changed"""
    rec = oracle_records(CASE_KEYWORDS, CASE_TEXT)
    want = near(rec, CASE_GROUPS, len(CASE_TEXT))
    _same(want, near_by_text(CASE_KEYWORDS, CASE_GROUPS, CASE_TEXT), "the two derivations")
    rec.setflags(write=False)
    want.setflags(write=False)
    return rec, want


def _dev(torch, arr):
    a = np.frombuffer(bytes(arr), dtype=np.uint8) if isinstance(arr, (bytes, bytearray)) else np.ascontiguousarray(arr)
    a = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])
    return torch.from_numpy(a.copy()).cuda()


def _rec_dev(torch, rec, room=None, fill=None):
    a = np.zeros(max(rec.size if room is None else room, 1), po.RECORD_DTYPE)
    if fill is not None:
        a["end_pos"] = fill
    a[:rec.size] = rec
    return torch.from_numpy(a.view(np.int64).reshape(-1, 2).copy()).cuda()


def _rec_host(t, n):
    return np.frombuffer(t[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()


def _same(got, want, what=None):
    assert got.size == want.size and np.array_equal(np.asarray(got).astype(po.RECORD_DTYPE), want), (what, got.size, want.size, got[:8], want[:8])


def _sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(DTYPE[sb])


def _join(plan, rec, ns, n_symbols, **kw):
    """Plan.near_records on the records `rec` (host): (the matches (host), the count)"""
    torch = __import__("torch")
    out, cnt = plan.near_records(_rec_dev(torch, rec), rec.size, ns, n_symbols, **kw)
    n = int(cnt.item())
    return _rec_host(out, min(n, out.shape[0])), n


def _scan(plan, dev, ns, capacity, **kw):
    """Plan.scan_near: (the matches (host), the count, the scan's count)"""
    out, cnt, found, _ = plan.scan_near(dev, ns, capacity=capacity, **kw)
    n = int(cnt.item())
    return _rec_host(out, min(n, out.shape[0])), n, int(found.item())


def _machine(keywords, sb=1, **kw):
    m = acm.Machine(sb, **kw)
    for w in keywords:
        m.add_keyword(_sym(w, sb) if sb > 1 else bytes(w))
    return m


def _byte_case(keywords, group_list, text, offsets=None):
    """(the oracle's records of the text, NEAR of them) for byte keywords: the two derivations must agree before
    anything else is compared"""
    rec = oracle_records(keywords, text)
    want = near(rec, group_list, len(text), offsets)
    _same(want, near_by_text(keywords, group_list, text, offsets), "the two derivations")
    return rec, want


def _shift(records, base):
    moved = records.copy()
    moved["end_pos"] += np.uint64(base)
    return moved


def _triples(records):
    return [tuple(int(x) for x in r) for r in records]


def test_the_case_is_not_trivial():
    per, ties, two, far, lost = case_facts(CASE_KEYWORDS, CASE_GROUPS, CASE_TEXT, CASE_CUT)
    print("matches per group %s, ties %d, ends with two anchors %d, of them with the window at the farther anchor %d, lost to the cut %d"
          % (per, ties, two, far, lost))
    assert per[5] == 0 and min(per[:5] + per[6:]) >= 2 and ties >= 2 and two >= 1 and far >= 1 and lost >= 1


def fixed_case_on_plan(torch, plan, sb, rec, want):
    """the fixed case through every call that takes a plan (of CASE_KEYWORDS as symbols of sb bytes, however it came to
    hold them: tests/test_growth_gpu.py calls this with grown plans); returns (symbols, set, offsets, NEAR under the cut)"""
    n = len(CASE_TEXT)
    ns = binding.NearSet(CASE_GROUPS)
    sym = _sym(CASE_TEXT, sb)
    dev = _dev(torch, sym)
    S = plan.near(ns)
    info = S.info()
    assert info == {"groups": 7, "terms": 19, "max_terms": 5, "max_width": 60, "max_postings": 3}   # disk, sda, timeout, retry: three groups each
    got, cnt, found = _scan(plan, dev, S, rec.size)
    assert found == rec.size and cnt == want.size
    _same(got, want, sb)
    # the join alone on the oracle's records, with the compiled set and with a set compiled for the call
    _same(_join(plan, rec, S, n)[0], want, sb)
    _same(_join(plan, rec, CASE_GROUPS, n)[0], want, sb)
    # one cut
    off = np.array([0, CASE_CUT, n], np.uint64)
    cut = near(rec, CASE_GROUPS, n, off)
    d_off = _dev(torch, off.astype(np.int64))
    _same(_join(plan, rec, S, n, offsets=d_off)[0], cut, sb)
    _same(_scan(plan, dev, S, rec.size, offsets=d_off)[0], cut, sb)
    # positions across 2^32 and with bit 63 set
    for base in BASES:
        _same(_scan(plan, dev, S, rec.size, pos_base=base)[0], _shift(want, base), (sb, base))
        _same(_join(plan, _shift(rec, base), S, n, pos_base=base, offsets=d_off)[0], _shift(cut, base), (sb, base))
    # host memory in, blocking
    _same(plan.scan_near_host(sym, ns), want, sb)
    _same(plan.scan_near_host(sym, ns, pos_base=BASES[0], offsets=off), _shift(cut, BASES[0]), sb)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_near_host(sym, ns, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW
    # an empty text, a text without a record
    assert plan.scan_near_host(np.zeros(0, DTYPE[sb]), ns).size == 0
    got, cnt, found = _scan(plan, _dev(torch, _sym(b"q" * 3000, sb)), S, 16)
    assert (cnt, found) == (0, 0)
    S.close()
    plan.status()
    return sym, ns, off, cut


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_the_fixed_case_on_every_symbol_size(torch_cuda, fixed, sb):
    rec, want = fixed
    m = _machine(CASE_KEYWORDS, sb)
    plan = m.plan(0)
    sym, ns, off, cut = fixed_case_on_plan(torch_cuda, plan, sb, rec, want)
    # the machine's own call on a GPU path
    _same(m.scan_near(sym, ns), want, sb)
    assert m.scan_path == PATH_GPU
    _same(m.scan_near(sym, ns, offsets=off), cut, sb)
    with pytest.raises(acm.ACMError) as e:
        m.scan_near(sym, ns, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW and m.scan_path == PATH_GPU
    plan.status()


def class_case(kat):
    """(comparator, text, the oracle's records under the comparator, NEAR of them): the fixed case in mixed case"""
    cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
    o = po.Oracle(1, po.MEYER85, cmp=cmp)
    for w in CASE_KEYWORDS:
        o.add_keyword(w)
    text = CASE_TEXT.replace(b"disk sda", b"DISK Sda").replace(b"she hers", b"SHE hers").replace(b"timeout error", b"TimeOut ERROR")
    assert text != CASE_TEXT and text.lower() == CASE_TEXT.lower()
    rec = o.scan(text)
    want = near(rec, CASE_GROUPS, len(text))
    _same(want, near_by_text(CASE_KEYWORDS, CASE_GROUPS, text.lower()), "the two derivations")
    assert near_by_text(CASE_KEYWORDS, CASE_GROUPS, text).size < want.size             # (the exact-case reading finds fewer)
    return cmp, text, rec, want


def class_case_on_plan(torch, plan, text, rec, want):
    """the mixed-case text through the calls that take a class plan of CASE_KEYWORDS"""
    got, cnt, found = _scan(plan, _dev(torch, text), CASE_GROUPS, rec.size)
    assert found == rec.size
    _same(got, want)
    _same(plan.scan_near_host(np.frombuffer(text, np.uint8), CASE_GROUPS), want)
    plan.status()


def test_a_class_plan_nears_over_classes(torch_cuda, kat):
    cmp, text, rec, want = class_case(kat)
    m = _machine(CASE_KEYWORDS, cmp=cmp)
    m.set_symbol_bytes(1)
    plan = m.plan_classes(0)
    class_case_on_plan(torch_cuda, plan, text, rec, want)
    _same(m.scan_near(text, CASE_GROUPS), want)
    assert m.scan_path == PATH_CLASSES
    plan.status()


def test_a_plan_with_a_pending_delta(torch_cuda):
    text = CASE_TEXT * 2
    m = _machine(CASE_KEYWORDS[:6])
    early = [([4, 5], 40, 0), ([0, 1, 3], 6, 2)]
    plan = m.plan(0)
    S0 = plan.near(early)
    for w in CASE_KEYWORDS[6:]:                                                         # the machine is ahead of the plan
        m.add_keyword(w)
    with pytest.raises(acm.ACMError) as e:
        plan.near(CASE_GROUPS)
    assert e.value.code == E_ARG                                                        # the plan does not know them yet
    plan.update(m)
    S = plan.near(CASE_GROUPS)
    rec, want = _byte_case(CASE_KEYWORDS, CASE_GROUPS, text)
    dev = _dev(torch_cuda, text)
    got, cnt, found = _scan(plan, dev, S, rec.size)
    assert found == rec.size
    _same(got, want)
    # the set made before the update stays valid: the keywords added since near nothing
    _same(_scan(plan, dev, S0, rec.size)[0], near_by_text(CASE_KEYWORDS, early, text))
    _same(m.scan_near(text, CASE_GROUPS), want)
    S.close()
    S0.close()
    plan.status()


def test_the_300_random_cases_with_cuts_and_empty_texts(torch_cuda):
    torch = torch_cuda
    plans = {}
    matches = cut_trials = 0
    for trial, (kws, group_list, text, offsets, rec, want) in enumerate(random_cases()):
        if tuple(kws) not in plans:                                                     # one plan per distinct dictionary
            plans[tuple(kws)] = _machine(kws).plan(0)
        plan = plans[tuple(kws)]
        what = (trial, kws, group_list, text, offsets)
        d_off = _dev(torch, offsets.astype(np.int64))
        _same(_join(plan, rec, group_list, len(text), offsets=d_off)[0], want, what)
        if trial % 3 == 0:
            got, cnt, found = _scan(plan, _dev(torch, text if text else b"\0"), group_list, max(rec.size, 1), offsets=d_off, n_symbols=len(text))
            assert found == rec.size
            _same(got, want, what)
        matches += want.size
        cut_trials += offsets.size > 2
    print("matches %d, trials with cuts %d, plans %d" % (matches, cut_trials, len(plans)))
    assert matches > 1000 and cut_trials > 100
    for plan in plans.values():
        plan.status()


def test_more_tiles_than_the_grid_has_blocks(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles, and
    walks reach across tile borders"""
    monkeypatch.setenv("ACM_GPU_NEAR_TILE", "64")
    kws = [b"a", b"b", b"ab", b"bbb"]
    group_list = [([0, 3], 9, 0), ([2, 3, 1], 6, 2), ([3], 3, 0), ([0, 1, 2, 3], 70, 0)]
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus + 3) * 64 + 65
    text = bytes(np.random.default_rng(8).choice(np.frombuffer(b"ab", np.uint8), size=n))
    rec = oracle_records(kws, text)
    assert rec.size > n
    want = near(rec, group_list, n)
    _same(near_by_text(kws, group_list, text[:1500]), want[want["end_pos"] < 1500], "the two derivations, where the slices are affordable")
    plan = _machine(kws).plan(0)
    got, cnt = _join(plan, rec, group_list, n)
    _same(got, want)
    assert want.size > n
    plan.status()


def test_long_walks_in_both_forms_give_the_definition(torch_cuda, monkeypatch):
    """some 600 x `a` with a rare `b` under the keywords a, aa, aaa, b: a head walks hundreds of records back to the
    last `b`, or to the begin of the text, or to its width; every walk cooperative, the default threshold of 64, and
    no walk cooperative"""
    kws = [b"a", b"aa", b"aaa", b"b"]
    text = bytearray(b"a" * 600)
    for at in (60, 61, 597):
        text[at] = ord("b")
    text = bytes(text)
    group_list = [([2, 3], 50, 0), ([2, 3], 400, 0), ([2, 3], WIDTH_MAX, 0), ([0, 1, 3], 50, 0), ([0, 1, 3], 400, 0), ([0, 1, 3], WIDTH_MAX, 0),
                  ([0, 1, 2, 3], WIDTH_MAX, 3)]
    rec = oracle_records(kws, text)
    want = near(rec, group_list, len(text))
    _same(near_by_text(kws, group_list[:1] + group_list[3:4], text), near(rec, group_list[:1] + group_list[3:4], len(text)), "the two derivations")
    per = np.bincount(want["keyword_id"], minlength=len(group_list))
    assert rec.size > 1700 and per.min() > 40 and int(want["length"].max()) > 400 and per[1] > per[0] and per[2] > per[1]
    plan = _machine(kws).plan(0)
    S = plan.near(group_list)
    dev = _dev(torch_cuda, text)
    off = np.array([0, 0, 130, 131, 599, 600], np.uint64)
    cut = near(rec, group_list, len(text), off)
    assert 0 < cut.size < want.size
    for coop in ("0", None, "2147483647"):
        if coop is None:
            monkeypatch.delenv("ACM_GPU_NEAR_COOP", raising=False)
        else:
            monkeypatch.setenv("ACM_GPU_NEAR_COOP", coop)
        _same(_join(plan, rec, S, len(text))[0], want, coop)
        _same(_scan(plan, dev, S, rec.size)[0], want, coop)
        # walks that end in the middle of a wave's round, and texts that cut them
        _same(_join(plan, rec, S, len(text), offsets=_dev(torch_cuda, off.astype(np.int64)))[0], cut, coop)
    S.close()
    plan.status()


@pytest.mark.parametrize("prefix", [61, 62, 63, 64])
def test_a_run_of_equal_ends_across_a_wave_boundary(torch_cuda, monkeypatch, prefix):
    """c, bc and abc end together behind `prefix` records of one symbol each: the three straddle the 64-record
    boundary of a wave, which is the tile's at ACM_GPU_NEAR_TILE=64 -- one record per group and end, from the head"""
    monkeypatch.setenv("ACM_GPU_NEAR_TILE", "64")
    kws = [b"c", b"bc", b"abc", b"x"]
    text = b"x" * prefix + b"abc" + b"xxabcx"
    group_list = [([0, 1, 2], 10, 2), ([2, 1, 0], 3, 0), ([3, 2], 5, 0), ([1, 3], 4, 1)]
    rec, want = _byte_case(kws, group_list, text)
    e = prefix + 2
    assert [int(r["end_pos"]) for r in rec[prefix:prefix + 3]] == [e, e, e]             # records prefix .. prefix + 2 end together
    assert _triples(want[want["end_pos"] == e]) == [(e, 4, 2), (e, 3, 1), (e, 2, 0), (e, 2, 3)]
    plan = _machine(kws).plan(0)
    for coop in ("0", "64"):
        monkeypatch.setenv("ACM_GPU_NEAR_COOP", coop)
        _same(_join(plan, rec, group_list, len(text))[0], want, (prefix, coop))
    _same(_scan(plan, _dev(torch_cuda, text), group_list, rec.size)[0], want, prefix)
    plan.status()


def test_early_arithmetic(torch_cuda):
    kws = [b"x", b"y"]
    plan = _machine(kws).plan(0)
    wide = [([0, 1], WIDTH_MAX, 0), ([1, 0], WIDTH_MAX, 1), ([1], 1, 0)]

    def run(text, group_list=wide, offsets=None):
        rec, want = _byte_case(kws, group_list, text, offsets)
        d_off = _dev(torch_cuda, np.array(offsets, np.int64)) if offsets is not None else None
        _same(_join(plan, rec, group_list, len(text), offsets=d_off)[0], want, text)
        _same(_scan(plan, _dev(torch_cuda, text), group_list, max(rec.size, 1), offsets=d_off)[0], want, text)
        for base in BASES:
            _same(_join(plan, _shift(rec, base), group_list, len(text), pos_base=base, offsets=d_off)[0], _shift(want, base), (text, base))
        return _triples(want)
    # an anchor at buffer index 0 .. 3 under the widest width: e + 1 - width lies in front of the buffer
    assert run(b"y") == [(0, 1, 1), (0, 1, 2)]
    assert run(b"xy") == [(0, 1, 1), (1, 2, 0), (1, 1, 1), (1, 1, 2)]
    assert run(b"x.y.")[1:] == [(2, 3, 0), (2, 1, 1), (2, 1, 2)]
    assert run(b"x..y")[1:] == [(3, 4, 0), (3, 1, 1), (3, 1, 2)]
    # a cut directly in front of and directly behind an anchor
    pair = [([0, 1], 9, 0)]
    assert run(b"x.y.x", pair) == [(2, 3, 0), (4, 3, 0)]
    assert run(b"x.y.x", pair, [0, 2, 5]) == [(4, 3, 0)]                                # ... | y.x
    assert run(b"x.y.x", pair, [0, 3, 5]) == [(2, 3, 0)]                                # x.y | .x
    assert run(b"x.y.x", pair, [0, 2, 3, 5]) == []
    plan.status()


def test_counts_on_the_device_and_a_scan_that_overflowed(torch_cuda, fixed):
    torch = torch_cuda
    rec, want = fixed
    n = len(CASE_TEXT)
    plan = _machine(CASE_KEYWORDS).plan(0)
    S = plan.near(CASE_GROUPS)
    sentinel = as_records([(SENTINEL, 7, 7)] * (want.size + 8))
    # out_capacity one short on the device: the count is exact, nothing is written at or behind out_capacity
    for cap in (want.size, want.size - 1, 1, 0):
        d_out = _rec_dev(torch, sentinel)
        out, c = plan.near_records(_rec_dev(torch, rec), rec.size, S, n, out=d_out, out_capacity=cap)
        host = _rec_host(d_out, sentinel.size)
        assert int(c.item()) == want.size and np.array_equal(host[cap:], sentinel[cap:]), cap
        if cap == want.size:
            _same(host[:cap], want)
    room = rec.size + 100

    def join(count):
        d_out = _rec_dev(torch, sentinel)
        d_rec = _rec_dev(torch, rec, room, fill=SENTINEL)
        out, cnt = plan.near_records(d_rec, room, S, n, out=d_out, out_capacity=want.size, count=torch.tensor([count], dtype=torch.int64, device="cuda"))
        return _rec_host(d_out, sentinel.size), int(cnt.item())
    out, cnt = join(rec.size)                                                           # d_n given: n is the room of the records
    _same(out[:cnt], want)
    assert np.array_equal(out[cnt:], sentinel[cnt:])
    out, cnt = join(room + 1)                                                           # *d_n > room: *d_count = 0 and nothing is written
    assert cnt == 0 and np.array_equal(out, sentinel)
    # the fused call with too little room for the scan's records: no match, *d_found suffices on repeat
    dev = _dev(torch, CASE_TEXT)
    got, cnt, found = _scan(plan, dev, S, rec.size - 1, out_capacity=want.size)
    assert cnt == 0 and found == rec.size
    got, cnt, found = _scan(plan, dev, S, found, out_capacity=want.size)
    _same(got, want)
    got, cnt, found = _scan(plan, dev, S, 0, out_capacity=want.size)                    # no room at all: the scan's count
    assert cnt == 0 and found == rec.size
    S.close()
    plan.status()


def test_near_device_arguments(torch_cuda, fixed):
    torch = torch_cuda
    rec, want = fixed
    n_symbols = len(CASE_TEXT)
    plan = _machine(CASE_KEYWORDS).plan(0)
    S = plan.near(CASE_GROUPS)
    L = acm.lib()
    assert want.size <= 2 * rec.size
    d_rec = _rec_dev(torch, rec, 3 * rec.size + want.size)
    sentinel = as_records([(SENTINEL, 7, 7)] * want.size)
    d_out = _rec_dev(torch, sentinel)
    count = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_near_tmp_bytes(plan.h, S.h, rec.size, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call(plan_h=plan.h, near_h=S.h, records=d_rec.data_ptr(), n=rec.size, out=d_out.data_ptr(), cap=want.size, cnt=count.data_ptr(),
             scratch=tmp.data_ptr(), tmp_bytes=tb, offsets=None, n_texts=0):
        return L.acm_gpu_near_records_device(plan_h, near_h, records, n, None, n_symbols, 0, offsets, n_texts, out, cap, cnt, scratch, tmp_bytes, None)
    assert tb > 0 and want.size > 0
    assert L.acm_gpu_near_tmp_bytes(plan.h, S.h, 1 << 31, 0) == 0 and L.acm_gpu_near_tmp_bytes(plan.h, None, 64, 0) == 0
    assert L.acm_gpu_scan_near_tmp_bytes(plan.h, S.h, 1 << 31, 64, 0) == 0 and L.acm_gpu_scan_near_tmp_bytes(plan.h, S.h, rec.size, n_symbols, 0) > tb
    assert call(plan_h=None) == E_ARG and call(near_h=None) == E_ARG and call(records=None) == E_ARG and call(out=None) == E_ARG
    assert call(cnt=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(cap=1 << 31) == E_ARG
    assert call(out=d_rec.data_ptr()) == E_ARG and call(out=d_rec.data_ptr() + 16 * (rec.size - 1)) == E_ARG     # d_out overlapping d_records
    assert call(offsets=d_rec.data_ptr(), n_texts=0) == E_ARG                          # no text, but symbols
    h = C.c_void_p()
    assert L.acm_gpu_near_create(plan.h, *binding.NearSet([([len(CASE_KEYWORDS)], 9, 0)]).args(), C.byref(h)) == E_ARG
    # a room beyond 2^40 slots (records x the most postings of a keyword), with fewer than 2^31 records
    crowd = plan.near([([0], 9, 0)] * 600)
    most = int(crowd.info()["max_postings"])
    assert most == 600
    n_beyond = -(-(1 << 40) // most)
    assert n_beyond < 1 << 31 and (n_beyond - 1) * most < 1 << 40 <= n_beyond * most
    assert L.acm_gpu_near_tmp_bytes(plan.h, crowd.h, n_beyond - 1, 0) > 0 and L.acm_gpu_near_tmp_bytes(plan.h, crowd.h, n_beyond, 0) == 0
    assert L.acm_gpu_scan_near_tmp_bytes(plan.h, crowd.h, n_beyond, 64, 0) == 0
    assert call(near_h=crowd.h, n=n_beyond) == E_ARG
    crowd.close()
    torch.cuda.synchronize()
    assert np.array_equal(_rec_host(d_out, want.size), sentinel) and int(count.item()) == 0x5A5A                  # nothing was touched
    assert call(out=d_rec.data_ptr() + 16 * rec.size) == 0                             # right behind the records: no overlap
    torch.cuda.synchronize()
    _same(_rec_host(d_rec[rec.size:], int(count.item())), want)
    assert call() == 0
    torch.cuda.synchronize()
    _same(_rec_host(d_out, int(count.item())), want)
    assert call(n=0, records=None, scratch=None, tmp_bytes=0) == 0                      # no record: no match
    torch.cuda.synchronize()
    assert int(count.item()) == 0
    S.close()
    plan.status()


def test_offsets_that_break_the_contract_match_nothing(torch_cuda, fixed):
    torch = torch_cuda
    rec, want = fixed
    n = len(CASE_TEXT)
    m = _machine(CASE_KEYWORDS)
    sentinel = as_records([(SENTINEL, 7, 7)] * want.size)
    for what, off in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]), ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n]), *broken_last_pair(n)):
        plan = m.plan(0)
        plan.status()
        d_out = _rec_dev(torch, sentinel)
        out, cnt = plan.near_records(_rec_dev(torch, rec), rec.size, CASE_GROUPS, n, offsets=_dev(torch, np.array(off, np.int64)), out=d_out)
        assert int(cnt.item()) == 0, what
        assert np.array_equal(_rec_host(d_out, want.size), sentinel), what
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_records_that_break_the_contract_are_skipped_and_reported(torch_cuda, fixed):
    rec, want = fixed
    m = _machine(CASE_KEYWORDS)
    pos_base = 1000
    shifted, moved = _shift(rec, pos_base), _shift(want, pos_base)
    kw = 5                                                                              # disk: a keyword of three groups
    bad = {"a start below pos_base": (pos_base + 2, 4, kw), "a length of 0": (pos_base + 20, 0, kw), "beyond the buffer": (pos_base + len(CASE_TEXT), 1, kw),
           "below pos_base": (pos_base - 1, 1, kw), "far beyond": (1 << 62, 3, kw),
           "a length of 0 where a head ends": (pos_base + int(rec["end_pos"][rec["keyword_id"] == 7][0]), 0, kw)}
    for what, triple in bad.items():
        plan = m.plan(0)
        plan.status()
        mixed = np.concatenate([shifted, np.array([triple], po.RECORD_DTYPE)])
        mixed = mixed[np.lexsort((-mixed["length"].astype(np.int64), mixed["end_pos"]))]   # canonical order with the stranger in it
        _same(_join(plan, mixed, CASE_GROUPS, len(CASE_TEXT), pos_base=pos_base)[0], moved, what)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()
