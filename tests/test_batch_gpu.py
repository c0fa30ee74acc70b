"""Batch scans on the GPU (acm_gpu_scan_batch_*, acm_scan_batch; csrc/dev_batch.h): many texts in one
buffer, every one scanned from the root on its own.  Every test is bit-exact on all three outputs
(records, text_id, first) against the ORACLE's scan of every text alone, shifted and concatenated
(tests/batch_cases.py) -- never against the library's own plain scan.  Every workload case first
shows, from the oracle alone, that it cannot pass trivially: the concatenation has strictly more
records than the batch (matches across a cut exist and must be dropped) and the batch has some."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, TEXTS, offsets_of, oracle_batch, oracle_batch_cut, random_cuts
from tests.cases import build_pair, build_pair_packed

pytestmark = pytest.mark.gpu


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


def _check_all(got, want, what=""):
    for g, w, name in zip(got, want, ("records", "text_id", "first")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g.shape, w.shape)


def _nontrivial(o, text, want):
    """from the oracle alone: matches across a cut exist (and are not the batch's), the batch is not empty"""
    whole = o.scan(text)
    print("batch records %d, dropped %d, in the concatenation %d" % (want[0].size, whole.size - want[0].size, whole.size))
    assert 0 < want[0].size < whole.size, (want[0].size, whole.size)
    return whole


def _three_ways(torch, plan, text, off, want, what=""):
    _check_all(plan.scan_batch(_dev(torch, text), _dev(torch, off)), want, what + " scan_batch")
    _check_all(plan.scan_batch_host(text, off), want, what + " scan_batch_host")


def test_boundary_cases_three_entry_points(torch_cuda):
    """cuts inside a keyword, right behind one and right in front of one, empty texts at the front, in
    the middle and at the end, nested suffix keywords"""
    m, o = build_pair(KEYWORDS, 1)
    want = oracle_batch(o, TEXTS)
    text = np.frombuffer(b"".join(TEXTS), np.uint8)
    _nontrivial(o, text, want)
    off = offsets_of(TEXTS)
    plan = m.plan(0)
    _three_ways(torch_cuda, plan, text, off, want)
    per_text = m.scan_batch(TEXTS)
    assert m.scan_path == 1 and len(per_text) == len(TEXTS)
    for t, text_t in enumerate(TEXTS):
        assert np.array_equal(per_text[t], o.scan(text_t) if len(text_t) else np.zeros(0, po.RECORD_DTYPE)), t
    # no text at all, and empty texts only
    _check_all(plan.scan_batch_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64)), oracle_batch(o, []))
    _check_all(plan.scan_batch_host(np.zeros(0, np.uint8), np.zeros(4, np.uint64)), oracle_batch(o, [b"", b"", b""]))
    _check_all(plan.scan_batch(_dev(torch_cuda, np.zeros(16, np.uint8))[:0], _dev(torch_cuda, np.zeros(4, np.uint64))),
               oracle_batch(o, [b"", b"", b""]))
    assert m.scan_batch([]) == []


def _kind(kind, monkeypatch, kat):
    """(machine, oracle, text, plan maker, check of the plan) of a plan kind"""
    n = 1 << 20
    if kind == "dense":
        kd, ko = acm.synth.keywords(1000)
        m, o = build_pair_packed(kd, ko)
        return m, o, acm.synth.text(n, kd, ko), m.plan, lambda p: p.info.kernel == 1
    if kind == "gram":
        kd, ko = acm.synth.keywords(20000)
        m, o = build_pair_packed(kd, ko, variant=po.MEYER85)
        return m, o, acm.synth.text(n, kd, ko), m.plan, lambda p: p.info.kernel == 5
    if kind == "csr":
        # the CSR walk is what a DENSE plan (no class table) launches on a text that is not 16-byte
        # aligned; plans of the other kinds copy such a text to an aligned buffer and run their own kernel
        kd, ko = acm.synth.keywords(1000)
        m, o = build_pair_packed(kd, ko)
        return m, o, acm.synth.text(n, kd, ko), m.plan, lambda p: p.info.kernel == 1 and p.info.records_direct == 0
    if kind in ("starts", "walk"):
        if kind == "walk":
            monkeypatch.setenv("ACM_GPU_SPARSE", "walk")
        kd, ko = acm.synth.keywords(2000, sym_bytes=4, vocab=500)
        m, o = build_pair_packed(kd, ko, sym_size=4)
        return m, o, acm.synth.text(n, kd, ko, sym_bytes=4, vocab=500), m.plan, lambda p: p.info.kernel == (3 if kind == "walk" else 4)
    if kind == "u64":
        rng = np.random.default_rng(8)
        vocab = rng.integers(0, 1 << 63, size=3000, dtype=np.uint64)
        kws = [vocab[rng.integers(0, vocab.size, size=rng.integers(1, 7))] for _ in range(1500)]
        m, o = build_pair(kws, 8)
        text = vocab[rng.integers(0, vocab.size, size=200003)]
        noise = rng.integers(0, text.size, size=20000)
        text[noise] = rng.integers(0, 1 << 63, size=noise.size, dtype=np.uint64)
        for _ in range(3000):
            w = kws[int(rng.integers(0, len(kws)))]
            at = int(rng.integers(0, text.size - w.size))
            text[at:at + w.size] = w
        return m, o, text, m.plan, lambda p: p.info.kernel == 4
    if kind == "classes":
        cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
        m = acm.Machine(1, cmp=cmp)
        o = po.Oracle(1, po.MEYER85, cmp=cmp)
        for kw in (b"He", b"SHE", b"his", b"hErs", b"Mrs", b"dalloway"):
            m.add_keyword(kw)
            o.add_keyword(kw)
        return m, o, None, m.plan_classes, lambda p: p.info.kernel == 1
    assert kind == "delta"
    kd, ko = acm.synth.keywords(450)
    m, o = build_pair_packed(kd[:ko[300]], ko[:301], variant=po.MEYER85)

    def plan_then_update(device):
        plan = m.plan(device)
        for k in range(300, 450):
            m.add_keyword(kd[ko[k]:ko[k + 1]])
            o.add_keyword(kd[ko[k]:ko[k + 1]])
        plan.update(m)
        return plan
    return m, o, acm.synth.text(n, kd, ko), plan_then_update, lambda p: p.info.delta_keywords == 150 and p.info.merges == 0


WORKLOAD = [(k, mean) for k in ("dense", "gram", "starts") for mean in (16, 64, 1024)] + [
    (k, 64) for k in ("walk", "csr", "u64", "classes", "delta")]


@pytest.mark.parametrize("kind,mean", WORKLOAD)
def test_plan_kinds_on_randomly_cut_text(torch_cuda, monkeypatch, kat, novel_bytes, kind, mean):
    """every plan kind: dense, 4-gram (with its short pass), start-parallel, sparse walk, CSR (a dense
    plan on a buffer that is not 16-byte aligned: the library has no per-scan report of the kernel it
    launched, so the case asserts the two facts the dispatch goes by -- a dense plan without a class
    table, a text pointer off the 16-byte grid -- and only the device call can reach it), 8-byte
    symbols, comparator classes, a plan with a pending delta"""
    m, o, text, make_plan, plan_ok = _kind(kind, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    if kind == "csr":
        text = text[1:]
    off = random_cuts(text.size, mean)
    assert np.any(off[1:] == off[:-1]) and off[1] == 0 and off[-2] == text.size        # empty texts, also first and last
    want = oracle_batch_cut(o, text, off)
    _nontrivial(o, text, want)
    if kind == "csr":
        dev = _dev(torch_cuda, np.concatenate([text[:1], text]))[1:]                    # 1 byte past a 16-byte boundary
        assert dev.data_ptr() % 16 == 1 and dev.is_contiguous()
        _check_all(plan.scan_batch(dev, _dev(torch_cuda, off)), want, kind)
    else:
        _three_ways(torch_cuda, plan, text, off, want, kind)


@pytest.mark.parametrize("kind", ["dense", "gram"])
def test_launch_seams_between_text_boundaries(torch_cuda, monkeypatch, kind):
    """launch segments of 8 KiB: text boundaries and launch seams interleave, keywords lie across both"""
    monkeypatch.setenv("ACM_GPU_SEGMENT_LOG2", "13")
    kd, ko = acm.synth.keywords(300 if kind == "dense" else 20000)
    m, o = build_pair_packed(kd, ko, variant=po.MEYER85)
    n = 9 * 8192 + 777
    text = acm.synth.text((n + 4095) // 4096 * 4096, kd, ko)[:n].copy()
    off = random_cuts(n, 64)
    for seam in range(8192, n, 8192):                    # a keyword across every seam, some of them cut there too
        text[seam - 5:seam + 7] = np.frombuffer(bytes(kd[ko[7]:ko[8]]) * 3, np.uint8)[:12]
    off = np.sort(np.concatenate([off, np.arange(8192, n, 16384, dtype=np.uint64)]))
    plan = m.plan(0)
    assert plan.info.kernel == (1 if kind == "dense" else 5)
    want = oracle_batch_cut(o, text, off)
    _nontrivial(o, text, want)
    _three_ways(torch_cuda, plan, text, off, want, kind)


def test_extreme_cuts_one_text_per_symbol_and_one_text_overall(torch_cuda):
    kd, ko = acm.synth.keywords(1000)
    m, o = build_pair_packed(kd, ko)
    for w in (b"a", b"ab"):
        m.add_keyword(w)
        o.add_keyword(w)
    n = 1 << 16
    text = acm.synth.text(n, kd, ko)
    plan = m.plan(0)
    # one text per symbol: every text is shorter than every keyword of 2 or more symbols
    off = np.arange(n + 1, dtype=np.uint64)
    want = oracle_batch_cut(o, text, off)
    whole = _nontrivial(o, text, want)
    assert np.all(want[0]["length"] == 1) and np.any(whole["length"] > 1)
    _three_ways(torch_cuda, plan, text, off, want, "per symbol")
    # one text overall: the plain ordered scan
    off = np.array([0, n], np.uint64)
    want = oracle_batch_cut(o, text, off)
    assert np.array_equal(want[0], whole) and np.array_equal(want[2], np.array([0, whole.size], np.uint64))
    _three_ways(torch_cuda, plan, text, off, want, "one text")


def _device_call(torch, plan, dev, off_dev, cap):
    L = acm.lib()
    n_sym, n_texts = dev.numel() * dev.element_size() // plan.sym_size, off_dev.numel() - 1
    rec = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device="cuda")
    tid = torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda")
    first = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_scan_batch_tmp_bytes(plan.h, cap, n_sym, n_texts)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_scan_batch_device(plan.h, dev.data_ptr(), n_sym, off_dev.data_ptr(), n_texts, rec.data_ptr(), tid.data_ptr(),
                                     first.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    n = int(cnt.item())
    got = None
    if rc == 0 and n <= cap:
        got = (np.frombuffer(rec[:n].cpu().numpy().tobytes(), dtype=binding.RECORD_DTYPE), tid[:n].cpu().numpy().view(np.uint32),
               first.cpu().numpy().view(np.uint64))
    return rc, n, got


@pytest.mark.parametrize("kind", ["dense", "gram"])
def test_overflow_reports_the_concatenations_count_which_suffices(torch_cuda, kind):
    kd, ko = acm.synth.keywords(1000 if kind == "dense" else 20000)
    m, o = build_pair_packed(kd, ko, variant=po.MEYER85)
    n = 1 << 18
    text = acm.synth.text(n, kd, ko)
    off = random_cuts(n, 64)
    want = oracle_batch_cut(o, text, off)
    whole = _nontrivial(o, text, want)
    plan = m.plan(0)
    dev, off_dev = _dev(torch_cuda, text), _dev(torch_cuda, off)
    for cap in (0, 1, want[0].size, whole.size - 1):     # (room for the batch's own records is not enough: the concatenation's are found first)
        rc, found, got = _device_call(torch_cuda, plan, dev, off_dev, cap)
        assert rc == 0 and found == whole.size and got is None, (cap, rc, found)
    rc, found, got = _device_call(torch_cuda, plan, dev, off_dev, whole.size)
    assert rc == 0 and found == want[0].size
    _check_all(got, want, "after overflow")
    plan.status()
    # the host call says so with its return value; the Python wrappers repeat the call once
    rec = np.zeros(4, binding.RECORD_DTYPE)
    nf = C.c_uint64(0)
    rc = acm.lib().acm_gpu_scan_batch_host(plan.h, text.ctypes.data, off.ctypes.data, off.size - 1, rec.ctypes.data, None, None, 4, C.byref(nf))
    assert rc == binding.ACM_GPU_E_OVERFLOW and nf.value == whole.size
    _check_all(plan.scan_batch(dev, off_dev, capacity=7), want, "retry")
    _check_all(plan.scan_batch_host(text, off, capacity=7), want, "retry host")


def test_bad_offsets_on_the_device_are_flagged_and_report_nothing(torch_cuda):
    kd, ko = acm.synth.keywords(1000)
    m, o = build_pair_packed(kd, ko)
    n = 1 << 18
    text = acm.synth.text(n, kd, ko)
    dev = _dev(torch_cuda, text)
    good = random_cuts(n, 64)
    for what in ("decreasing", "first", "last"):
        off = good.copy()
        if what == "decreasing":
            off[100], off[101] = good[101] + 5, good[100]
            assert off[100] > off[101]
        elif what == "first":
            off[:3] = 1
        else:
            off[-2:] = n - 1
        plan = m.plan(0)
        rc, found, got = _device_call(torch_cuda, plan, dev, _dev(torch_cuda, off), 4096)
        assert rc == 0 and found == 0, (what, rc, found)
        with pytest.raises(binding.ACMError) as e:
            plan.status()
        assert e.value.code == -7, what
        # the host call refuses the same offsets before anything is uploaded (it has no n_symbols
        # argument: there the last offset IS the number of symbols, so "last" is no violation)
        if what == "last":
            continue
        nf = C.c_uint64(0)
        rec = np.zeros(4096, binding.RECORD_DTYPE)
        assert acm.lib().acm_gpu_scan_batch_host(plan.h, text.ctypes.data, off.ctypes.data, off.size - 1, rec.ctypes.data, None, None, 4096,
                                                 C.byref(nf)) == binding.ACM_GPU_E_ARG
    # a plan that was given good offsets stays clean
    plan = m.plan(0)
    rc, found, got = _device_call(torch_cuda, plan, dev, _dev(torch_cuda, good), 4096)
    assert rc == 0 and found > 0
    plan.status()
    # and so do the other argument checks: too many texts, too little scratch
    L = acm.lib()
    assert L.acm_gpu_scan_batch_device(plan.h, dev.data_ptr(), n, _dev(torch_cuda, good).data_ptr(), 1 << 32, None, None, None, 0,
                                       _dev(torch_cuda, np.zeros(1, np.uint64)).data_ptr(), dev.data_ptr(), 1 << 18, None) == binding.ACM_GPU_E_ARG
    cnt = torch_cuda.zeros(1, dtype=torch_cuda.int64, device="cuda")
    assert L.acm_gpu_scan_batch_device(plan.h, dev.data_ptr(), n, _dev(torch_cuda, good).data_ptr(), good.size - 1, None, None, None, 0,
                                       cnt.data_ptr(), dev.data_ptr(), 16, None) == binding.ACM_GPU_E_ARG
