"""Per-keyword tallies on the GPU (acm_gpu_tally_*, acm_tally; csrc/dev_tally.h).  The expected answer
is always np.bincount over the ORACLE's records (tests/tally_cases.py), never the library's own
scan; every workload case first shows from the oracle alone that it cannot pass trivially (two
keywords with different non-zero counts, one keyword without a match).

Not here: a tally of a hand-made record buffer that holds a keyword id the plan does not have (the
error flag, the id never used as an index).  The kernel's launcher would have to be exported from the
product library for that test alone."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.cases import build_pair
from tests.tally_cases import FORM_GLOBAL, FORM_LDS, KINDS, PATH_CLASSES, PATH_GPU, kind, nontrivial, oracle_tally, prefilled

pytestmark = pytest.mark.gpu

E_ARG = binding.ACM_GPU_E_ARG


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


def _host(t):
    return t.cpu().numpy().view(np.uint64).copy()


def _device_tally(torch, plan, dev, K, **kw):
    """Plan.tally into counters pre-filled with a pattern: (what was added, total, need, the counters)"""
    counters = _dev(torch, prefilled(K))
    got, total, need = plan.tally(dev, tally=counters, **kw)
    assert got is counters
    return _host(counters) - prefilled(K), total, need, _host(counters)


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind_three_entry_points(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram (20,000 keywords: the global form), CSR (a dense plan on a pointer off the 16-byte
    grid, also at every window), start-parallel, sparse walk, 8-byte symbols, comparator classes, a
    plan with a pending delta -- through Plan.tally (four windows or more), Plan.tally_host and Machine.tally"""
    m, o, text, make_plan, plan_ok, form = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    assert plan.tally_form == form and plan.tally_keywords == o.nb_keywords
    if name == "csr":
        text = text[1:]
    want, n_records = oracle_tally(o, text)
    nontrivial(want)
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([text[:1], text]))[1:]                    # 1 byte past a 16-byte boundary
        assert dev.data_ptr() % 16 == 1 and dev.is_contiguous()
    else:
        dev = _dev(torch_cuda, text)
    window, capacity = 1 << 16, 1 << 16
    assert text.size > 1.5 * window
    added, total, need, _ = _device_tally(torch_cuda, plan, dev, want.size, window=window, capacity=capacity)
    print("total %d, largest window %d" % (total, need))
    assert 0 < need <= capacity and total == n_records
    assert np.array_equal(added, want)
    plan.status()
    got, total = plan.tally_host(text)
    assert total == n_records and np.array_equal(got, want)
    got, total = m.tally(text)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    assert total == n_records and np.array_equal(got, want)
    got2, total = m.tally(text, tally=got)                                                # the machine's counters are added to as well
    assert got2 is got and total == n_records and np.array_equal(got, 2 * want)


def test_both_kernel_forms_on_the_same_input(torch_cuda, monkeypatch, kat):
    m, o, text, make_plan, plan_ok, form = kind("dense", monkeypatch, kat)
    text = text[:1 << 18]
    want, n_records = oracle_tally(o, text)
    nontrivial(want)
    plan = make_plan(0)
    dev = _dev(torch_cuda, text)
    assert plan.tally_form == FORM_LDS
    lds = _device_tally(torch_cuda, plan, dev, want.size, window=1 << 16, capacity=1 << 14)
    monkeypatch.setenv("ACM_GPU_TALLY", "global")
    assert plan.tally_form == FORM_GLOBAL
    glob = _device_tally(torch_cuda, plan, dev, want.size, window=1 << 16, capacity=1 << 14)
    for added, total, need, _ in (lds, glob):
        assert total == n_records and 0 < need <= 1 << 14 and np.array_equal(added, want)
    assert lds[2] == glob[2]
    plan.status()


LONG = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMN"          # 40 symbols


def test_window_cuts_lose_and_double_nothing(torch_cuda):
    keywords = [b"he", b"she", b"hers", b"s", LONG]
    assert len(LONG) == 40
    # the long keyword from offset 10 (across 16, 32 and 48), from 100 (across 112 and 128) and ending with the text
    text = b"ushers he " + LONG + b" she sells hers; his ushers she hers ssh" + b"x" * 10 + LONG + b" hers she " * 9 + b"she" + LONG
    assert text[10:50] == LONG and text[100:140] == LONG and len(text) % 16 and 200 < len(text) < 400
    m, o = build_pair(keywords, 1)
    whole, _ = oracle_tally(o, text)
    assert np.unique(whole).size >= 3 and whole[4] == 3
    plan = m.plan(0)
    n = len(text)
    dev = _dev(torch_cuda, text)
    for window in (16, 48, 4096):
        for emit_from in (0, 17, n - 1, n):
            want, n_records = oracle_tally(o, text, emit_from=emit_from)
            added, total, need, _ = _device_tally(torch_cuda, plan, dev, len(keywords), emit_from=emit_from, window=window, capacity=4096)
            assert total == n_records and np.array_equal(added, want), (window, emit_from, added, want)
            assert need <= n_records and (need > 0) == (n_records > 0)
    # an empty text, and texts shorter than one window
    empty = _dev(torch_cuda, np.zeros(16, np.uint8))[:0]
    added, total, need, _ = _device_tally(torch_cuda, plan, empty, len(keywords), window=16, capacity=64)
    assert total == 0 and need == 0 and not added.any()
    got, total = plan.tally_host(np.zeros(0, np.uint8))
    assert total == 0 and not got.any()
    for short in (b"she", b"ushers hers"):
        want, n_records = oracle_tally(o, short)
        added, total, need, _ = _device_tally(torch_cuda, plan, _dev(torch_cuda, short), len(keywords), window=16, capacity=64)
        assert n_records > 0 and total == need == n_records and np.array_equal(added, want)
        got, total = plan.tally_host(np.frombuffer(short, np.uint8))
        assert total == n_records and np.array_equal(got, want)
    plan.status()


def test_overflow_is_all_or_nothing(torch_cuda, monkeypatch):
    text = b"a" * 65536
    m, o = build_pair([b"a", b"aa", b"aaa"], 1)
    rec = o.scan(text)
    assert np.all(np.bincount(rec["end_pos"].astype(np.int64))[2:] == 3)               # 3 records per position from index 2 on
    want = np.bincount(rec["keyword_id"], minlength=3).astype(np.uint64)
    assert want.tolist() == [65536, 65535, 65534]                                          # (every keyword matches here: the counts differ)
    per_window = np.bincount((rec["end_pos"] // 4096).astype(np.int64))
    plan = m.plan(0)
    dev = _dev(torch_cuda, text)
    added, total, need, counters = _device_tally(torch_cuda, plan, dev, 3, window=4096, capacity=4096)
    assert need == per_window.max() == 4096 * 3 and need > 4096
    assert total == 0 and np.array_equal(counters, prefilled(3))                           # bit-identical
    # the stated bound: window x M records cannot overflow; 65,536 adds on each of three addresses
    added, total, need, _ = _device_tally(torch_cuda, plan, dev, 3, window=4096, capacity=4096 * 3)
    assert need == 4096 * 3 and total == rec.size and np.array_equal(added, want)
    monkeypatch.setenv("ACM_GPU_TALLY", "global")
    added, total, need, _ = _device_tally(torch_cuda, plan, dev, 3, window=4096, capacity=4096 * 3)
    assert need == 4096 * 3 and total == rec.size and np.array_equal(added, want)
    monkeypatch.delenv("ACM_GPU_TALLY")
    # the host call with room for 4,096 records: one window of the whole text overflows, the call repeats itself
    # with windows of 4,096 / 3 symbols
    monkeypatch.setenv("ACM_GPU_TALLY_CAPACITY", "4096")
    got, total = plan.tally_host(np.frombuffer(text, np.uint8))
    assert total == rec.size and np.array_equal(got, want)
    monkeypatch.setenv("ACM_GPU_TALLY_CAPACITY", "2")                                      # less than 16 x M: the capacity grows
    got, total = plan.tally_host(np.frombuffer(text[:5000], np.uint8))
    assert total == 3 * 5000 - 3 and got.tolist() == [5000, 4999, 4998]
    plan.status()


def test_tally_accumulates_over_calls_and_over_pieces(torch_cuda, monkeypatch, kat):
    m, o, text, make_plan, plan_ok, form = kind("dense", monkeypatch, kat)
    want, n_records = oracle_tally(o, text)
    nontrivial(want)
    plan = make_plan(0)
    half, warm = text.size // 2 + 5, m.lmax - 1
    assert warm >= 8
    # a keyword across the cut, so that the second piece's warm-up matters
    kd, ko = acm.synth.keywords(1000)
    kw = kd[ko[3]:ko[4]]
    text = text.copy()
    text[half - 3:half - 3 + kw.size] = kw
    want, n_records = oracle_tally(o, text)
    first, n_first = oracle_tally(o, text[:half])
    assert n_first < n_records and first[3] + 1 <= want[3]
    dev = _dev(torch_cuda, text)
    counters = _dev(torch_cuda, prefilled(want.size))
    _, t1, _ = plan.tally(dev[:half], tally=counters, window=1 << 17, capacity=1 << 14)
    assert t1 == n_first and np.array_equal(_host(counters) - prefilled(want.size), first)
    _, t2, _ = plan.tally(dev[half - warm:], emit_from=warm, tally=counters, window=1 << 17, capacity=1 << 14)
    assert t1 + t2 == n_records and np.array_equal(_host(counters) - prefilled(want.size), want)
    plan.status()


@pytest.mark.parametrize("name", ["dense", "gram"])
def test_total_equals_plan_count(torch_cuda, monkeypatch, kat, name):
    m, o, text, make_plan, plan_ok, form = kind(name, monkeypatch, kat)
    text = text[:1 << 18]
    want, n_records = oracle_tally(o, text)
    nontrivial(want)
    plan = make_plan(0)
    assert plan_ok(plan) and plan.tally_form == form
    dev = _dev(torch_cuda, text)
    for emit_from in (0, 70001):
        want, n_records = oracle_tally(o, text, emit_from=emit_from)
        added, total, need, _ = _device_tally(torch_cuda, plan, dev, want.size, emit_from=emit_from, window=1 << 16, capacity=1 << 14)
        assert total == int(plan.count(dev, emit_from=emit_from).item()) == n_records == int(added.sum())
        assert np.array_equal(added, want)
    plan.status()


def test_tally_device_arguments(torch_cuda):
    m, o = build_pair([b"he", b"she"], 1)
    plan = m.plan(0)
    L = acm.lib()
    dev = _dev(torch_cuda, b"ushers" * 10)
    counters = _dev(torch_cuda, prefilled(2))
    out = torch_cuda.zeros(2, dtype=torch_cuda.int64, device="cuda")
    tb = L.acm_gpu_tally_tmp_bytes(plan.h, 16, 64)
    assert tb >= 64 * 16 + 2 * 8
    tmp = torch_cuda.empty(tb, dtype=torch_cuda.uint8, device="cuda")

    def call(n_keywords=2, window=16, capacity=64, tmp_bytes=tb, tally=counters.data_ptr()):
        return L.acm_gpu_tally_device(plan.h, dev.data_ptr(), dev.numel(), 0, tally, n_keywords, window, capacity, out.data_ptr(),
                                      out.data_ptr() + 8, tmp.data_ptr(), tmp_bytes, None)
    assert call(window=0) == E_ARG and call(window=24) == E_ARG
    assert call(capacity=0) == E_ARG and call(capacity=1 << 31) == E_ARG
    assert call(n_keywords=1) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(tally=None) == E_ARG
    assert L.acm_gpu_tally_tmp_bytes(plan.h, 16, 0) == 0 and L.acm_gpu_tally_tmp_bytes(plan.h, 16, 1 << 31) == 0
    torch_cuda.cuda.synchronize()
    assert np.array_equal(_host(counters), prefilled(2))
    assert call(window=64) == 0                                                            # one window
    torch_cuda.cuda.synchronize()
    assert (_host(counters) - prefilled(2)).tolist() == [10, 10] and out.cpu().tolist() == [20, 20]
    plan.status()
