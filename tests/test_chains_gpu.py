"""Keyword chains with bounded gaps on the GPU (acm_gpu_chains_*, acm_gpu_scan_chains_*, acm_scan_chains;
csrc/dev_chains.h).  The expected answer is always the definition of CHAINS in plain Python over the ORACLE's
records (tests/chain_cases.py) and, for byte text, a second derivation from the text alone with `re` -- never
the library's own scan or join.  All comparisons are exact, order included.  Texts are a few hundred symbols;
one case has more records than the capped grid has tiles of 64, so that blocks stride over tiles, and one has
windows of hundreds of records, so that the wave walks them."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import broken_last_pair, offsets_of
from tests.chain_cases import (CASE_CHAINS, CASE_CUT, CASE_KEYWORDS, CASE_TEXT, as_records, case_facts, chain_terms, chains, chains_by_re,
                               fixed_offset_patterns, oracle_records, random_case)
from tests.tally_cases import PATH_CLASSES, PATH_GPU

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
SENTINEL = 0x0123456789ABCDEF
AB_WORDS = [b"a", b"b", b"aa", b"ab", b"ba", b"bb", b"aaa", b"aab", b"aba", b"abb", b"baa", b"bab", b"bba", b"bbb"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def fixed():
    """(the oracle's records of the fixed case, CHAINS of them): computed once, never changed"""
    rec = oracle_records(CASE_KEYWORDS, CASE_TEXT)
    want = chains(rec, CASE_CHAINS, len(CASE_TEXT))
    _same(want, chains_by_re(CASE_KEYWORDS, CASE_CHAINS, CASE_TEXT), "the two derivations")
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


def _join(plan, rec, cs, n_symbols, **kw):
    """Plan.chains_records on the records `rec` (host): (the matches (host), the count)"""
    torch = __import__("torch")
    out, cnt = plan.chains_records(_rec_dev(torch, rec), rec.size, cs, n_symbols, **kw)
    n = int(cnt.item())
    return _rec_host(out, min(n, out.shape[0])), n


def _scan(plan, dev, cs, capacity, **kw):
    """Plan.scan_chains: (the matches (host), the count, the scan's count)"""
    out, cnt, found, _ = plan.scan_chains(dev, cs, capacity=capacity, **kw)
    n = int(cnt.item())
    return _rec_host(out, min(n, out.shape[0])), n, int(found.item())


def _machine(keywords, sb=1, **kw):
    m = acm.Machine(sb, **kw)
    for w in keywords:
        m.add_keyword(_sym(w, sb) if sb > 1 else bytes(w))
    return m


def _byte_case(keywords, chain_list, text, offsets=None):
    """(machine, the oracle's records of the text, CHAINS of them) for byte keywords: the two derivations must
    agree before anything else is compared"""
    rec = oracle_records(keywords, text)
    want = chains(rec, chain_list, len(text), offsets)
    _same(want, chains_by_re(keywords, chain_list, text, offsets), "the two derivations")
    return _machine(keywords), rec, want


def _triples(records):
    return [tuple(int(x) for x in r) for r in records]


def test_the_case_is_not_trivial():
    per, ties, several, ruled_out, lost = case_facts(CASE_KEYWORDS, CASE_CHAINS, CASE_TEXT, CASE_CUT)
    print("matches per chain %s, ties %d, ends with several starts %d, ruled out by a middle gap %d, lost to the cut %d"
          % (per, ties, several, ruled_out, lost))
    assert min(per) >= 2 and ties >= 2 and several >= 1 and ruled_out >= 1 and lost >= 1


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_the_fixed_case_on_every_symbol_size(torch_cuda, fixed, sb):
    torch = torch_cuda
    rec, want = fixed
    n = len(CASE_TEXT)
    m = _machine(CASE_KEYWORDS, sb)
    specs = [[y for j, (k, gmin, gmax) in enumerate(terms) for y in ([(gmin, gmax)] if j else []) + [_sym(CASE_KEYWORDS[k], sb)]] for terms in CASE_CHAINS]
    cs = binding.ChainSet.from_specs(m, specs)                      # (the machine holds every keyword: the ids are CASE_KEYWORDS')
    assert m.nb_keywords == len(CASE_KEYWORDS) and chain_terms(cs) == [list(t) for t in CASE_CHAINS]
    own = rec
    plan = m.plan(0)
    sym = _sym(CASE_TEXT, sb)
    dev = _dev(torch, sym)
    S = plan.chains_create(cs)
    info = S.info()
    assert info["chains"] == len(CASE_CHAINS) and info["terms"] == cs.terms.shape[0] and info["max_terms"] == 3 and info["max_gap"] == 40
    assert info["max_postings"] == 3 and info["max_last_postings"] == 3          # `1.1` ends three chains
    got, cnt, found = _scan(plan, dev, S, rec.size)
    assert found == rec.size and cnt == want.size
    _same(got, want, sb)
    # the join alone on the oracle's records, with the compiled set and with a set compiled for the call
    _same(_join(plan, own, S, n)[0], want, sb)
    _same(_join(plan, own, cs, n)[0], want, sb)
    # nonzero pos_base
    moved, shifted = want.copy(), own.copy()
    moved["end_pos"] += 5000
    shifted["end_pos"] += 5000
    _same(_scan(plan, dev, S, rec.size, pos_base=5000)[0], moved, sb)
    _same(_join(plan, shifted, S, n, pos_base=5000)[0], moved, sb)
    # host memory in, blocking; the machine's own call on a GPU path
    _same(plan.scan_chains_host(sym, cs), want, sb)
    _same(plan.scan_chains_host(sym, cs, pos_base=5000), moved, sb)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_chains_host(sym, cs, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW
    _same(m.scan_chains(sym, cs), want, sb)
    assert m.scan_path == PATH_GPU
    with pytest.raises(acm.ACMError) as e:
        m.scan_chains(sym, cs, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW
    # out_capacity one short on the device: the count is exact, nothing is written at or behind out_capacity
    sentinel = as_records([(SENTINEL, 7, 7)] * (want.size + 8))
    for cap in (want.size, want.size - 1, 1, 0):
        d_out = _rec_dev(torch, sentinel)
        out, c = plan.chains_records(_rec_dev(torch, own), own.size, S, n, out=d_out, out_capacity=cap)
        host = _rec_host(d_out, sentinel.size)
        assert int(c.item()) == want.size and np.array_equal(host[cap:], sentinel[cap:]), cap
        if cap == want.size:
            _same(host[:cap], want)
    # an empty text, a text without a record
    assert plan.scan_chains_host(np.zeros(0, DTYPE[sb]), cs).size == 0
    got, cnt, found = _scan(plan, _dev(torch, _sym(b"q" * 3000, sb)), S, 16)
    assert (cnt, found) == (0, 0)
    S.close()
    plan.status()


def test_gap_boundaries(torch_cuda):
    kws = [b"x", b"y", b"ab", b"bc"]
    plan = _machine(kws).plan(0)

    def run(text, chain_list):
        m, rec, want = _byte_case(kws, chain_list, text)
        _same(_join(plan, rec, chain_list, len(text))[0], want, text)
        _same(_scan(plan, _dev(torch_cuda, text), chain_list, max(rec.size, 1))[0], want, text)
        return _triples(want)
    gap = [[(0, 0, 0), (1, 2, 4)]]                                                # x .{2,4} y
    assert run(b"x.y", gap) == [] and run(b"x..y", gap) == [(3, 4, 0)] and run(b"x....y", gap) == [(5, 6, 0)] and run(b"x.....y", gap) == []
    assert run(b"xy x.y", [[(0, 0, 0), (1, 0, 0)]]) == [(1, 2, 0)]                # gap 0 means adjacent
    assert run(b"abc", [[(2, 0, 0), (3, 0, 0)]]) == []                            # ab, bc on abc: terms never overlap
    assert run(b"abbc", [[(2, 0, 0), (3, 0, 0)]]) == [(3, 4, 0)]
    assert run(b"x.y", [[(0, 0, 0), (1, 0, 9)]]) == [(2, 3, 0)]                   # a first term at buffer index 0: s - 1 - gap_max clamps
    assert run(b"y.x", [[(0, 0, 0), (1, 0, 9)]]) == []                            # a second term at index 0: nothing lies in front
    assert run(b"xy", [[(0, 0, 0), (1, 1, 9)]]) == []                             # s = 1 with gap_min 1: the window is empty
    plan.status()


def test_set_shapes(torch_cuda):
    kws = [b"a", b"b", b"ab"]
    plan = _machine(kws).plan(0)
    text = b"aabab.aaab..a.a.a.ab ba" * 3

    def run(chain_list, text=text):
        m, rec, want = _byte_case(kws, chain_list, text)
        S = plan.chains_create(chain_list)
        _same(_join(plan, rec, S, len(text))[0], want, chain_list)
        _same(_scan(plan, _dev(torch_cuda, text), S, rec.size)[0], want, chain_list)
        info = S.info()
        S.close()
        return want, info
    # a chain of 16 terms: as many level passes
    want, info = run([[(0, 0, 0)] + [(j % 2, 0, 3) for j in range(1, 16)]], b"ab" * 9 + b" " + b"a.b.." * 9 + b" abab")
    assert want.size >= 2 and info["max_terms"] == 16
    # one keyword at three levels of one chain
    want, info = run([[(0, 0, 0), (0, 0, 2), (0, 0, 2)]])
    assert want.size >= 6 and info["max_postings"] == 3 and info["max_last_postings"] == 1
    # one keyword in several chains and at the end of several: ties of different chains at one end come out in order
    want, info = run([[(0, 0, 0), (1, 0, 3)], [(2, 0, 0), (1, 0, 6)], [(1, 0, 0)], [(0, 0, 0), (0, 0, 1), (1, 0, 2)], [(1, 0, 0), (0, 1, 4)]])
    groups = np.unique(want["end_pos"], return_counts=True)[1]
    assert groups.max() >= 4 and info["max_last_postings"] == 4 and info["max_postings"] == 5
    # a chain of one term gives its keyword's records
    want, info = run([[(2, 0, 0)]])
    rec = oracle_records(kws, text)
    _same(want, as_records([(int(r["end_pos"]), 2, 0) for r in rec if r["keyword_id"] == 2]))
    plan.status()


def test_150_random_cases_with_cuts_and_empty_texts(torch_cuda):
    torch = torch_cuda
    plan = _machine(AB_WORDS).plan(0)
    rng = np.random.default_rng(2026)
    matches = cut_trials = 0
    for trial in range(150):
        kws, chain_list, text, offsets = random_case(rng)
        mapped = [[(AB_WORDS.index(kws[k]), a, b) for k, a, b in terms] for terms in chain_list]
        rec = oracle_records(AB_WORDS, text)
        want = chains(rec, mapped, len(text), offsets)
        _same(want, chains_by_re(kws, chain_list, text, offsets), (trial, "the two derivations"))
        what = (trial, kws, chain_list, text, offsets)
        d_off = _dev(torch, offsets.astype(np.int64))
        _same(_join(plan, rec, mapped, len(text), offsets=d_off)[0], want, what)
        if trial % 3 == 0:
            got, cnt, found = _scan(plan, _dev(torch, text if text else b"\0"), mapped, max(rec.size, 1), offsets=d_off, n_symbols=len(text))
            assert found == rec.size
            _same(got, want, what)
        matches += want.size
        cut_trials += offsets.size > 2
    print("matches %d, trials with cuts %d" % (matches, cut_trials))
    assert matches > 500 and cut_trials > 50
    plan.status()


def test_both_walk_forms_give_the_definition(torch_cuda, monkeypatch):
    """400 x `a` with keywords a, aa: a window of gap_max 300 holds some 600 records, so that the wave form strides it
    several times; every window cooperative, the default threshold of 64, and no window cooperative"""
    kws = [b"a", b"aa"]
    text = b"a" * 400
    chain_list = [[(0, 0, 0), (1, 0, 300)], [(1, 0, 0), (0, 100, 300), (1, 0, 300)], [(0, 0, 0), (0, 20, 31), (1, 65, 300)], [(1, 0, 0), (1, 0, 3)]]
    m, rec, want = _byte_case(kws, chain_list, text)
    assert rec.size == 799 and want.size > 1000
    plan = m.plan(0)
    S = plan.chains_create(chain_list)
    dev = _dev(torch_cuda, text)
    for coop in ("0", None, "1000000000"):
        if coop is None:
            monkeypatch.delenv("ACM_GPU_CHAINS_COOP", raising=False)
        else:
            monkeypatch.setenv("ACM_GPU_CHAINS_COOP", coop)
        _same(_join(plan, rec, S, len(text))[0], want, coop)
        _same(_scan(plan, dev, S, rec.size)[0], want, coop)
    # windows that end in the middle of a wave's stride, and texts that cut them
    off = np.array([0, 0, 130, 131, 399, 400], np.uint64)
    cut = chains(rec, chain_list, len(text), off)
    assert 0 < cut.size < want.size
    for coop in ("0", "1000000000"):
        monkeypatch.setenv("ACM_GPU_CHAINS_COOP", coop)
        _same(_join(plan, rec, S, len(text), offsets=_dev(torch_cuda, off.astype(np.int64)))[0], cut, coop)
    S.close()
    plan.status()


def test_more_tiles_than_the_grid_has_blocks(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles, and
    windows reach across tile borders"""
    monkeypatch.setenv("ACM_GPU_CHAINS_TILE", "64")
    kws = [b"a", b"b", b"ab"]
    chain_list = [[(0, 0, 0), (1, 1, 3)], [(2, 0, 0), (2, 0, 5), (0, 0, 1)], [(1, 0, 0), (1, 40, 70)]]
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus + 3) * 64 + 65
    text = bytes(np.random.default_rng(8).choice(np.frombuffer(b"ab", np.uint8), size=n))
    rec = oracle_records(kws, text)
    assert rec.size > n
    want = chains_by_re(kws, chain_list, text)
    _same(chains(rec[rec["end_pos"] < 2000], chain_list, 2000), want[want["end_pos"] < 2000], "the two derivations, where the loop is affordable")
    plan = _machine(kws).plan(0)
    got, cnt = _join(plan, rec, chain_list, n)
    _same(got, want)
    assert n // 2 < want.size
    plan.status()


def test_a_packed_batch_equals_its_texts_one_by_one(torch_cuda):
    texts = [b"", b"GET /x", b" HTTP/1.1", b"GET /id=4 HTTP/1.1 Host: a:1", b"", b"", b"/", b"1.1", b"Host::", b"GET / HTTP/1.1"] * 6 + [b""]
    packed = b"".join(texts)
    off = offsets_of(texts)
    m, rec, want = _byte_case(CASE_KEYWORDS, CASE_CHAINS, packed, off)
    whole = chains(rec, CASE_CHAINS, len(packed))
    # `GET /x| HTTP/1.1`: GET .{2,40} HTTP would span the cut; `/|1.1`: so would / 1.1
    spanning = set(_triples(whole)) - set(_triples(want))
    assert {c for _, _, c in spanning} >= {0, 2} and (10, 11, 0) in spanning and 0 < want.size < whole.size
    plan = m.plan(0)
    one_by_one = []
    for t, text in enumerate(texts):
        if text:
            got = plan.scan_chains_host(np.frombuffer(text, np.uint8), CASE_CHAINS, pos_base=int(off[t]))
            one_by_one.append(got)
    _same(np.concatenate(one_by_one), want, "the texts one by one")
    dev, d_off = _dev(torch_cuda, packed), _dev(torch_cuda, off.astype(np.int64))
    _same(_join(plan, rec, CASE_CHAINS, len(packed), offsets=d_off)[0], want)
    _same(_join(plan, rec, CASE_CHAINS, len(packed))[0], whole)
    got, cnt, found = _scan(plan, dev, CASE_CHAINS, rec.size, offsets=d_off)
    assert found == rec.size
    _same(got, want)
    _same(plan.scan_chains_host(np.frombuffer(packed, np.uint8), CASE_CHAINS, offsets=off), want)
    _same(m.scan_chains(packed, CASE_CHAINS, offsets=off), want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_chains_host(np.frombuffer(packed, np.uint8), CASE_CHAINS, offsets=[0, 9, 5, len(packed)])
    assert e.value.code == E_ARG
    plan.status()                                                                       # a record across a cut is no error


def test_counts_on_the_device_and_a_scan_that_overflowed(torch_cuda, fixed):
    torch = torch_cuda
    rec, want = fixed
    n = len(CASE_TEXT)
    plan = _machine(CASE_KEYWORDS).plan(0)
    S = plan.chains_create(CASE_CHAINS)
    sentinel = as_records([(SENTINEL, 7, 7)] * (want.size + 8))
    room = rec.size + 100

    def join(count):
        d_out = _rec_dev(torch, sentinel)
        d_rec = _rec_dev(torch, rec, room, fill=SENTINEL)
        out, cnt = plan.chains_records(d_rec, room, S, n, out=d_out, out_capacity=want.size, count=torch.tensor([count], dtype=torch.int64, device="cuda"))
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
    # arguments
    L = acm.lib()
    assert L.acm_gpu_chains_tmp_bytes(plan.h, S.h, rec.size, 0) > 0 and L.acm_gpu_chains_tmp_bytes(plan.h, S.h, 1 << 31, 0) == 0
    assert L.acm_gpu_chains_tmp_bytes(plan.h, None, 64, 0) == 0 and L.acm_gpu_scan_chains_tmp_bytes(plan.h, S.h, 1 << 31, 64, 0) == 0
    d_rec = _rec_dev(torch, rec, 2 * rec.size)
    count = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_chains_tmp_bytes(plan.h, S.h, rec.size, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call(chains_h=S.h, out=d_rec.data_ptr() + 16 * rec.size, cap=rec.size, tmp_bytes=tb, cnt=count.data_ptr()):
        return L.acm_gpu_chains_records_device(plan.h, chains_h, d_rec.data_ptr(), rec.size, None, n, 0, None, 0, out, cap, cnt, tmp.data_ptr(), tmp_bytes, None)
    assert call(chains_h=None) == E_ARG and call(out=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(cnt=None) == E_ARG
    assert call(out=d_rec.data_ptr() + 16 * (rec.size - 1)) == E_ARG and call(cap=1 << 31) == E_ARG      # d_out overlapping d_records
    h = C.c_void_p()
    assert L.acm_gpu_chains_create(plan.h, *binding.ChainSet([[(len(CASE_KEYWORDS), 0, 0)]]).args(), C.byref(h)) == E_ARG
    torch.cuda.synchronize()
    assert int(count.item()) == 0x5A5A                                                  # nothing was touched
    assert want.size <= rec.size and call() == 0                                        # right behind the records: no overlap
    torch.cuda.synchronize()
    _same(_rec_host(d_rec[rec.size:], int(count.item())), want)
    S.close()
    plan.status()


def test_chains_device_arguments(torch_cuda, fixed):
    torch = torch_cuda
    rec, want = fixed
    n_symbols = len(CASE_TEXT)
    plan = _machine(CASE_KEYWORDS).plan(0)
    S = plan.chains_create(CASE_CHAINS)
    L = acm.lib()
    d_rec = _rec_dev(torch, rec, 2 * rec.size + want.size)
    sentinel = as_records([(SENTINEL, 7, 7)] * want.size)
    d_out = _rec_dev(torch, sentinel)
    count = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_chains_tmp_bytes(plan.h, S.h, rec.size, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call(plan_h=plan.h, chains_h=S.h, records=d_rec.data_ptr(), n=rec.size, out=d_out.data_ptr(), cap=want.size, cnt=count.data_ptr(),
             scratch=tmp.data_ptr(), tmp_bytes=tb, offsets=None, n_texts=0):
        return L.acm_gpu_chains_records_device(plan_h, chains_h, records, n, None, n_symbols, 0, offsets, n_texts, out, cap, cnt, scratch, tmp_bytes, None)
    assert tb > 0 and want.size > 0
    assert call(plan_h=None) == E_ARG and call(chains_h=None) == E_ARG and call(records=None) == E_ARG and call(out=None) == E_ARG
    assert call(cnt=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(cap=1 << 31) == E_ARG
    assert call(out=d_rec.data_ptr()) == E_ARG and call(out=d_rec.data_ptr() + 16 * (rec.size - 1)) == E_ARG     # d_out overlapping d_records
    assert call(out=d_rec.data_ptr() - 16 * (want.size - 1)) == E_ARG
    assert call(offsets=d_rec.data_ptr(), n_texts=0) == E_ARG                          # no text, but symbols
    # a room beyond CHAINS_MOST_SLOTS = 2^40 state slots (records x the most postings of a keyword), with fewer than 2^31 records
    crowd = plan.chains_create([[(0, 0, 0)]] * 600)
    most = int(crowd.info()["max_postings"])
    assert most == 600
    n_beyond = -(-(1 << 40) // most)
    assert n_beyond < 1 << 31 and (n_beyond - 1) * most < 1 << 40 <= n_beyond * most
    assert L.acm_gpu_chains_tmp_bytes(plan.h, crowd.h, n_beyond - 1, 0) > 0 and L.acm_gpu_chains_tmp_bytes(plan.h, crowd.h, n_beyond, 0) == 0
    assert L.acm_gpu_scan_chains_tmp_bytes(plan.h, crowd.h, n_beyond, 64, 0) == 0
    assert call(chains_h=crowd.h, n=n_beyond) == E_ARG
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
        out, cnt = plan.chains_records(_rec_dev(torch, rec), rec.size, CASE_CHAINS, n, offsets=_dev(torch, np.array(off, np.int64)), out=d_out)
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
    shifted, moved = rec.copy(), want.copy()
    shifted["end_pos"] += pos_base
    moved["end_pos"] += pos_base
    kw = 1                                                                              # HTTP: a keyword in the middle and at the end of chains
    bad = {"a start below pos_base": (pos_base + 2, 4, kw), "a length of 0": (pos_base + 20, 0, kw), "beyond the buffer": (pos_base + len(CASE_TEXT), 1, kw),
           "below pos_base": (pos_base - 1, 1, kw), "far beyond": (1 << 62, 3, kw)}
    for what, triple in bad.items():
        plan = m.plan(0)
        plan.status()
        mixed = np.concatenate([shifted, np.array([triple], po.RECORD_DTYPE)])
        mixed = mixed[np.lexsort((-mixed["length"].astype(np.int64), mixed["end_pos"]))]   # canonical order with the stranger in it
        _same(_join(plan, mixed, CASE_CHAINS, len(CASE_TEXT), pos_base=pos_base)[0], moved, what)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_fixed_gaps_equal_patterns_on_the_same_device_records(torch_cuda):
    torch = torch_cuda
    kws = [b"ab", b"bc", b"x", b"y"]
    text = b"ab.bc abxbc abbc ab..bc xabybc xaby.bc abab.bc" * 5
    fixed_chains = [[(0, 0, 0), (1, 1, 1)], [(2, 0, 0), (0, 0, 0), (3, 0, 0)], [(0, 0, 0), (1, 0, 0)], [(0, 0, 0), (0, 0, 0), (1, 1, 1)], [(3, 0, 0)]]
    pats = fixed_offset_patterns(kws, fixed_chains)
    m, rec, want = _byte_case(kws, fixed_chains, text)
    assert np.all(np.bincount(want["keyword_id"], minlength=len(fixed_chains)) >= 5)
    plan = m.plan(0)
    d_rec = _rec_dev(torch, rec)
    got_c, n_c = plan.chains_records(d_rec, rec.size, fixed_chains, len(text))
    got_p, n_p = plan.patterns_records(d_rec, rec.size, pats, len(text))
    assert int(n_c.item()) == int(n_p.item()) == want.size
    _same(_rec_host(got_c, want.size), _rec_host(got_p, want.size))
    _same(_rec_host(got_c, want.size), want)
    plan.status()


def test_a_class_plan_chains_over_classes(torch_cuda, kat):
    cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
    m, o = _machine(CASE_KEYWORDS, cmp=cmp), po.Oracle(1, po.MEYER85, cmp=cmp)
    for w in CASE_KEYWORDS:
        o.add_keyword(w)
    m.set_symbol_bytes(1)
    text = CASE_TEXT.replace(b"GET /c", b"get /c").replace(b"Host: y", b"HOST: y").replace(b"HTTP/1.0", b"http/1.0")
    assert text != CASE_TEXT and text.lower() == CASE_TEXT.lower()
    rec = o.scan(text)
    want = chains(rec, CASE_CHAINS, len(text))
    lowered = [w.lower() for w in CASE_KEYWORDS]
    _same(want, chains_by_re(lowered, CASE_CHAINS, text.lower()), "the two derivations")
    assert chains_by_re(CASE_KEYWORDS, CASE_CHAINS, text).size < want.size             # (the exact-case reading finds fewer)
    plan = m.plan_classes(0)
    got, cnt, found = _scan(plan, _dev(torch_cuda, text), CASE_CHAINS, rec.size)
    assert found == rec.size
    _same(got, want)
    _same(plan.scan_chains_host(np.frombuffer(text, np.uint8), CASE_CHAINS), want)
    _same(m.scan_chains(text, CASE_CHAINS), want)
    assert m.scan_path == PATH_CLASSES
    plan.status()


def test_a_plan_with_a_pending_delta(torch_cuda):
    text = CASE_TEXT * 2
    m = _machine(CASE_KEYWORDS[:3])
    early = [[(0, 0, 0), (1, 2, 40)]]                                                   # GET .{2,40} HTTP
    plan = m.plan(0)
    S0 = plan.chains_create(early)
    for w in CASE_KEYWORDS[3:]:                                                         # the machine is ahead of the plan
        m.add_keyword(w)
    with pytest.raises(acm.ACMError) as e:
        plan.chains_create(CASE_CHAINS)
    assert e.value.code == E_ARG                                                        # the plan does not know them yet
    plan.update(m)
    S = plan.chains_create(CASE_CHAINS)
    rec = oracle_records(CASE_KEYWORDS, text)
    want = chains(rec, CASE_CHAINS, len(text))
    _same(want, chains_by_re(CASE_KEYWORDS, CASE_CHAINS, text), "the two derivations")
    dev = _dev(torch_cuda, text)
    got, cnt, found = _scan(plan, dev, S, rec.size)
    assert found == rec.size
    _same(got, want)
    # the set made before the update stays valid: the keywords added since chain nothing
    _same(_scan(plan, dev, S0, rec.size)[0], chains_by_re(CASE_KEYWORDS, early, text))
    _same(m.scan_chains(text, CASE_CHAINS), want)
    S.close()
    S0.close()
    plan.status()
