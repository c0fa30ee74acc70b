"""Per-text keyword counts of a batch on the GPU (acm_gpu_tally_batch_*, acm_tally_batch;
csrc/dev_tally_batch.h).  The expected matrix is always derived from the ORACLE's scan of every text
alone (tests/tally_batch_cases.py: np.unique over text_id << 32 | keyword_id), never from the
library's own scan; every workload case first shows from the oracle alone that it cannot pass
trivially."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import KEYWORDS, offsets_of, random_cuts
from tests.cases import build_pair
from tests.grep_cases import GREP_TEXTS, oracle_hits
from tests.tally_batch_cases import check, dense, expected, nontrivial, window_pairs
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind, oracle_tally

pytestmark = pytest.mark.gpu

E_ARG = binding.ACM_GPU_E_ARG
GUARD = 0x5A


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


def _np(g):
    """a TalliedBatch of device tensors -> one of numpy arrays cut to size"""
    return binding.TalliedBatch(g.row_ptr.cpu().numpy().view(np.uint64).copy(), g.col[:g.nnz].cpu().numpy().view(np.uint32).copy(),
                                g.val[:g.nnz].cpu().numpy().view(np.uint64).copy(), g.nnz, g.total, g.need, g.need_pairs)


def _texts(text, off):
    o = [int(x) for x in off]
    return [text[o[t]:o[t + 1]] for t in range(len(o) - 1)]


@pytest.fixture(scope="module")
def boundary():
    """(machine, oracle, plan, text, offsets, expected) of the boundary set on a dense plan, made once"""
    m, o = build_pair(KEYWORDS, 1)
    text = np.frombuffer(b"".join(GREP_TEXTS), np.uint8)
    off = offsets_of(GREP_TEXTS)
    want = expected(o, text, off)
    nontrivial(o, text, off, want)
    plan = m.plan(0)
    assert plan.info.kernel == 1, plan.describe()
    return m, o, plan, text, off, want


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind_three_entry_points(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram, CSR (a dense plan on a pointer off the 16-byte grid, also at every window),
    start-parallel, sparse walk, 8-byte symbols, comparator classes, a plan with a pending delta --
    through Plan.tally_batch (four windows or more, one text over three whole windows),
    Plan.tally_batch_host and Machine.tally_batch"""
    m, o, text, make_plan, plan_ok, form = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    if name == "csr":
        text = text[1:]
    window = capacity = 1 << 16
    assert text.size > 3 * window
    off = random_cuts(text.size, 700)
    # one text covers the windows 1, 2 and 3 (the 8-byte kind's 200,003 symbols end inside window 3: its text runs to the end)
    off = off[(off < window) | (off >= min(4 * window, text.size))]
    assert np.any(off[1:] == off[:-1]) and off[0] == 0 and off[-1] == text.size
    want = expected(o, text, off)
    nontrivial(o, text, off, want, window=window)
    records = int(want[2].sum())
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([np.zeros(1, text.dtype), text]))[1:]
        assert dev.data_ptr() % 16 == 1
    else:
        dev = _dev(torch_cuda, text)
    g = plan.tally_batch(dev, _dev(torch_cuda, off), window=window, capacity=capacity, pair_capacity=records)
    print("entries %d, total %d, largest window %d, partial pairs %d" % (g.nnz, g.total, g.need, g.need_pairs))
    assert 0 < g.need <= capacity and window_pairs(o, text, off, window).shape[0] <= g.need_pairs <= records
    check(_np(g), want, "%s Plan.tally_batch" % name)
    plan.status()
    check(plan.tally_batch_host(text, off), want, "%s Plan.tally_batch_host" % name)
    check(m.tally_batch(_texts(text, off)), want, "%s Machine.tally_batch" % name)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    plan.status()


REPEATED = b"ushers he she hers " * 40                                     # 760 symbols: 48 windows of 16, four keywords in each


@pytest.mark.parametrize("slots,row", [(None, None), (8, None), (None, 4), (8, 4)])
def test_small_shapes_table_flushes_and_wide_rows(torch_cuda, monkeypatch, boundary, slots, row):
    """windows of 16 symbols; a table of 8 slots flushes several times per block and leaves duplicate
    partial pairs of one key; R = 4 sends every row of more than 4 partial pairs to the wide-row form.
    All four settings give the oracle's matrix, so the same one."""
    m, o, plan, text, off, want = boundary
    if slots:
        monkeypatch.setenv("ACM_GPU_TALLY_BATCH_SLOTS", str(slots))
    if row:
        monkeypatch.setenv("ACM_GPU_TALLY_BATCH_ROW", str(row))
    g = plan.tally_batch(_dev(torch_cuda, text), _dev(torch_cuda, off), window=16, capacity=64, pair_capacity=int(want[2].sum()))
    assert 0 < g.need <= 64
    check(_np(g), want, ("boundary set", slots, row))
    check(plan.tally_batch_host(text, off), want, ("boundary set, host", slots, row))
    # the boundary set with a text of 48 windows in the middle: a row of far more than 4 partial pairs
    texts = GREP_TEXTS[:7] + [REPEATED] + GREP_TEXTS[7:]
    long_text, long_off = np.frombuffer(b"".join(texts), np.uint8), offsets_of(texts)
    long_want = expected(o, long_text, long_off)
    nontrivial(o, long_text, long_off, long_want, window=16)
    g = plan.tally_batch(_dev(torch_cuda, long_text), _dev(torch_cuda, long_off), window=16, capacity=64, pair_capacity=int(long_want[2].sum()))
    least = window_pairs(o, long_text, long_off, 16).shape[0]               # every window of the long text leaves its own pairs
    assert g.need_pairs >= least > 4 * long_want[1].size
    check(_np(g), long_want, ("long row", slots, row))
    plan.status()


def test_a_hot_key(torch_cuda):
    """one text of 65,536 times the same one-symbol keyword: every lane of every wave on one slot"""
    m, o = build_pair([b"a", b"b"], 1)
    plan = m.plan(0)
    text = np.frombuffer(b"a" * 65536, np.uint8)
    off = np.array([0, 65536], np.uint64)
    want = expected(o, text, off)
    assert want[0].tolist() == [0, 1] and want[1].tolist() == [0] and want[2].tolist() == [65536]
    for window, capacity in ((4096, 4096), (1 << 16, 1 << 16)):
        g = plan.tally_batch(_dev(torch_cuda, text), _dev(torch_cuda, off), window=window, capacity=capacity, pair_capacity=4096)
        assert g.need == window and 0 < g.need_pairs <= 4096
        check(_np(g), want, ("hot key", window))
    check(plan.tally_batch_host(text, off), want, "hot key, host")
    plan.status()


def _raw(torch, plan, dev, d_off, n_texts, window, capacity, pair_capacity, room):
    """acm_gpu_tally_batch_device into arrays of `room` entries filled with guard values;
    (rc, res = [nnz, total, need, need_pairs], row_ptr, col, val)"""
    L = acm.lib()
    n = dev.numel()
    row_ptr = torch.full((n_texts + 1,), GUARD, dtype=torch.int64, device="cuda")
    col = torch.full((room,), GUARD, dtype=torch.int32, device="cuda")
    val = torch.full((room,), GUARD, dtype=torch.int64, device="cuda")
    res = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_tally_batch_tmp_bytes(plan.h, window, capacity, pair_capacity, n, n_texts)
    tmp = torch.empty(max(tb, 16), dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_tally_batch_device(plan.h, dev.data_ptr(), n, d_off.data_ptr(), n_texts, window, capacity, pair_capacity, row_ptr.data_ptr(),
                                      col.data_ptr(), val.data_ptr(), res.data_ptr(), res.data_ptr() + 8, res.data_ptr() + 16,
                                      res.data_ptr() + 24, tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    return rc, res.cpu().tolist(), row_ptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()


def test_overflow_protocols_and_guards(torch_cuda, boundary):
    torch = torch_cuda
    m, o, plan, text, off, want = boundary
    dev, d_off = _dev(torch, text), _dev(torch, off)
    n_texts, nnz, records = off.size - 1, want[1].size, int(want[2].sum())
    assert records > nnz > 1
    # a window with more records than room: nothing but the need
    g = plan.tally_batch(dev, d_off, window=16, capacity=1, pair_capacity=records)
    assert g.need > 1 and g.nnz == 0 and g.total == 0
    # more partial pairs than room: the number of kept records of the call, exactly; a repeat with it succeeds
    g = plan.tally_batch(dev, d_off, window=16, capacity=64, pair_capacity=1)
    assert g.nnz == 0 and g.total == 0 and g.need_pairs == records and 0 < g.need <= 64
    g = plan.tally_batch(dev, d_off, window=16, capacity=64, pair_capacity=g.need_pairs)
    check(_np(g), want, "the repeat")
    # guard values behind nnz stay on success; nothing is written on a pair overflow
    rc, res, row_ptr, col, val = _raw(torch, plan, dev, d_off, n_texts, 16, 64, records, records + 8)
    assert rc == 0 and res[0] == nnz and res[1] == records and 0 < res[2] <= 64 and nnz <= res[3] <= records
    assert np.array_equal(row_ptr.view(np.uint64), want[0]) and np.array_equal(col[:nnz].view(np.uint32), want[1])
    assert np.array_equal(val[:nnz].view(np.uint64), want[2]) and np.all(col[nnz:] == GUARD) and np.all(val[nnz:] == GUARD)
    rc, res, row_ptr, col, val = _raw(torch, plan, dev, d_off, n_texts, 16, 64, 1, 8)
    assert rc == 0 and res[0] == 0 and res[1] == 0 and res[3] == records
    assert np.all(row_ptr == GUARD) and np.all(col == GUARD) and np.all(val == GUARD)
    plan.status()
    # arguments
    L = acm.lib()
    assert L.acm_gpu_tally_batch_tmp_bytes(plan.h, 16, 0, 8, text.size, n_texts) == 0
    assert L.acm_gpu_tally_batch_tmp_bytes(plan.h, 16, 64, 0, text.size, n_texts) == 0
    assert L.acm_gpu_tally_batch_tmp_bytes(plan.h, 16, 64, 1 << 31, text.size, n_texts) == 0
    assert L.acm_gpu_tally_batch_tmp_bytes(plan.h, 16, 64, 8, text.size, 1 << 31) == 0
    for window, capacity, pairs in ((0, 64, 8), (24, 64, 8), (16, 0, 8), (16, 1 << 31, 8), (16, 64, 0), (16, 64, 1 << 31)):
        tmp = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
        out = torch.zeros(64, dtype=torch.int64, device="cuda")
        p = out.data_ptr()
        assert L.acm_gpu_tally_batch_device(plan.h, dev.data_ptr(), dev.numel(), d_off.data_ptr(), n_texts, window, capacity, pairs, p, p + 128,
                                            p + 256, p + 384, p + 392, p + 400, p + 408, tmp.data_ptr(), tmp.numel(), None) == E_ARG


def test_bad_offsets(torch_cuda):
    torch = torch_cuda
    m, o = build_pair([b"he", b"she"], 1)
    dev = _dev(torch, b"ushers" * 10)
    n = dev.numel()
    # offsets that break the contract, all of them inside the buffer's range: the error flag, all counts 0, no array written
    for what, bad in (("decreasing", [0, 40, 30, n]), ("last", [0, 30, 30, n - 1]), ("first", [1, 30, 30, n])):
        fresh = m.plan(0)
        rc, res, row_ptr, col, val = _raw(torch, fresh, dev, _dev(torch, np.array(bad, np.uint64)), 3, 16, 64, 64, 64)
        assert rc == 0, what
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        assert res[0] == 0 and res[1] == 0 and res[3] == 0, (what, res)
        assert np.all(row_ptr == GUARD) and np.all(col == GUARD) and np.all(val == GUARD), what
    # the same plan kind with good offsets
    plan = m.plan(0)
    rc, res, row_ptr, col, val = _raw(torch, plan, dev, _dev(torch, np.array([0, 30, 30, n], np.uint64)), 3, 16, 64, 64, 64)
    assert rc == 0 and res[:2] == [4, 20] and row_ptr.tolist() == [0, 2, 2, 4] and col[:4].tolist() == [0, 1, 0, 1] and val[:4].tolist() == [5] * 4
    plan.status()


def test_no_text_at_all(torch_cuda, boundary):
    torch = torch_cuda
    m, o, plan, text, off, want = boundary
    empty = _dev(torch, np.zeros(16, np.uint8))[:0]
    g = plan.tally_batch(empty, _dev(torch, np.zeros(1, np.uint64)), window=16, capacity=64)
    assert (g.nnz, g.total, g.need, g.need_pairs) == (0, 0, 0, 0) and g.row_ptr.cpu().tolist() == [0]
    h = plan.tally_batch_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert (h.nnz, h.total) == (0, 0) and h.row_ptr.tolist() == [0] and h.col.size == 0 and h.val.size == 0
    assert m.tally_batch([]).row_ptr.tolist() == [0]
    # texts, all of them empty
    g = plan.tally_batch(empty, _dev(torch, np.zeros(4, np.uint64)), window=16, capacity=64)
    assert (g.nnz, g.total, g.need) == (0, 0, 0) and g.row_ptr.cpu().tolist() == [0, 0, 0, 0]
    plan.status()


def test_to_sparse_csr(torch_cuda, boundary):
    torch = torch_cuda
    m, o, plan, text, off, want = boundary
    g = plan.tally_batch(_dev(torch, text), _dev(torch, off), window=16, capacity=64, pair_capacity=int(want[2].sum()))
    s = g.to_sparse_csr(len(KEYWORDS))
    assert s.layout == torch.sparse_csr and s.is_cuda and tuple(s.shape) == (off.size - 1, len(KEYWORDS))
    assert s.crow_indices().data_ptr() == g.row_ptr.data_ptr() and s.col_indices().data_ptr() == g.col.data_ptr()      # built in place
    assert s.values().data_ptr() == g.val.data_ptr()
    assert np.array_equal(s.to_dense().cpu().numpy(), dense(want, len(KEYWORDS)))
    h = plan.tally_batch_host(text, off).to_sparse_csr(len(KEYWORDS))
    assert np.array_equal(h.to_dense().numpy(), dense(want, len(KEYWORDS)))


def test_composition_with_tally_and_grep(torch_cuda, boundary):
    torch = torch_cuda
    m, o, plan, text, off, want = boundary
    g = _np(plan.tally_batch(_dev(torch, text), _dev(torch, off), window=16, capacity=64, pair_capacity=int(want[2].sum())))
    K = len(KEYWORDS)
    per_keyword = np.bincount(g.col, weights=g.val.astype(np.float64), minlength=K).astype(np.uint64)
    alone, from_oracle = np.zeros(K, np.uint64), np.zeros(K, np.uint64)
    for t in _texts(text, off):
        if t.size:
            alone += plan.tally(_dev(torch, t), window=16, capacity=64)[0].cpu().numpy().view(np.uint64)[:K]
            from_oracle += oracle_tally(o, t)[0]
    assert np.array_equal(per_keyword, alone) and np.array_equal(per_keyword, from_oracle)
    row_sums = np.add.reduceat(np.concatenate([g.val, [0]]).astype(np.uint64), np.minimum(g.row_ptr[:-1].astype(np.int64), g.nnz))
    row_sums[np.diff(g.row_ptr.astype(np.int64)) == 0] = 0
    assert np.array_equal(row_sums, oracle_hits(o, text, off))
    plan.status()
