"""The keyword co-occurrence matrix of a batch on the GPU (acm_gpu_cooccur_*, acm_cooccur; csrc/dev_cooccur.h).  The
expected matrix is always the brute force of the definition over the ORACLE's count matrix (tests/cooccur_cases.py over
tests/tally_batch_cases.expected), or over a matrix the test itself wrote, never over the library's own counts; every
workload first shows from the oracle alone that it cannot pass trivially."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import offsets_of, random_cuts
from tests.cases import build_pair
from tests.cooccur_cases import (ALL_FLAGS, DIAGONAL, EXAMPLE, EXAMPLE_KEYWORDS, EXAMPLE_LIMIT3, EXAMPLE_TEXTS, MASK, PRODUCT, Expected, add_expected,
                                 brute_force, check, cooccurred_of, cut_rows, matrix_of, nontrivial, tallied_of)
from tests.tally_batch_cases import expected
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind
from tests.test_score_gpu import _dev, _matrix, _texts

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
K = len(EXAMPLE_KEYWORDS)
N = len(EXAMPLE_TEXTS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def example():
    """(machine, plan, text, offsets, the oracle's count matrix) of the worked example on a dense plan, made once"""
    m, o = build_pair(EXAMPLE_KEYWORDS, 1)
    text = np.frombuffer(b"".join(EXAMPLE_TEXTS), np.uint8)
    off = offsets_of(EXAMPLE_TEXTS)
    counts = expected(o, text, off)
    for flags in ALL_FLAGS:
        want = brute_force(counts, K, flags)
        assert (want.cross, want.nnz, want.co_ptr.tolist(), want.entries()) == EXAMPLE[flags]
    plan = m.plan(0)
    assert plan.info.kernel == 1, plan.describe()
    return m, plan, text, off, counts


def _device_matrix(torch, e):
    """an Expected as a Cooccurred of device tensors (the input of an ADD on the device)"""
    def some(a):
        return _dev(torch, a) if a.size else torch.zeros(1, dtype={4: torch.int32, 8: torch.int64}[a.itemsize], device="cuda")
    return binding.Cooccurred(_dev(torch, e.co_ptr), some(e.co_col), some(e.co_val), e.nnz, e.cross, e.skipped, e.flags)


@pytest.mark.parametrize("limit", [0, 3])
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_the_example_through_the_four_routes(torch_cuda, example, flags, limit):
    """the worked example of the header in windows of 16 symbols"""
    torch = torch_cuda
    m, plan, text, off, counts = example
    want = nontrivial(counts, brute_force(counts, K, flags, limit))
    if flags == 0 and limit == 3:
        assert (want.cross, want.nnz, want.skipped, want.entries()) == EXAMPLE_LIMIT3
    records = int(counts[2].sum())
    dev, d_off = _dev(torch, text), _dev(torch, off)
    g = plan.cooccur_matrix(_matrix(torch, tallied_of(counts)), flags, limit)
    check(g, want, ("Plan.cooccur_matrix", flags, limit))
    assert g.total is None and g.flags == flags
    plan.status()
    g = plan.cooccur(dev, d_off, flags, limit, window=16, capacity=64, pair_capacity=records)
    assert 0 < g.need <= 64 and g.total == records
    check(g, want, ("Plan.cooccur", flags, limit))
    dense = g.to_sparse_csr(K).to_dense().cpu().numpy()
    assert np.array_equal(dense.astype(np.uint64), np.array([[want.entries().get((a, b), 0) for b in range(K)] for a in range(K)], np.uint64))
    ids, values = g.row(0)
    assert ids.cpu().tolist() == [b for (a, b) in sorted(want.entries()) if a == 0] and g.value(3, 2) == g.value(2, 3) == want.entries()[(2, 3)]
    plan.status()
    g = plan.cooccur(dev, d_off, flags, limit, window=16, capacity=64, pair_capacity=records, cross_capacity=want.cross, out_capacity=want.nnz)
    check(g, want, ("Plan.cooccur, exact rooms", flags, limit))
    got = plan.cooccur_host(text, off, flags, limit)
    check(got, want, ("Plan.cooccur_host", flags, limit))
    assert got.total == records
    plan.status()
    got = m.cooccur(EXAMPLE_TEXTS, flags, limit)
    check(got, want, ("Machine.cooccur", flags, limit))
    assert m.scan_path == PATH_GPU and got.total == records
    # more keywords than the plan has: empty rows behind
    check(plan.cooccur(dev, d_off, flags, limit, n_keywords=K + 3, window=16, capacity=64), brute_force(counts, K + 3, flags, limit), ("K + 3", flags, limit))
    plan.status()


@pytest.fixture(scope="module")
def triangle():
    """a caller's matrix whose rows have 0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 300 entries: both sides of a
    wave, of a block of the expansion and of the float root's exact range; row t begins at keyword 7 t mod 40, so that
    pairs repeat between the rows.  (counts, {flags: Expected})"""
    sizes = [0, 1, 2, 3, 63, 64, 65, 0, 127, 128, 129, 255, 256, 257, 300, 2, 0]
    rng = np.random.default_rng(11)
    rows = [{(7 * t) % 40 + i: int(rng.integers(1, 1 << 30)) for i in range(r)} for t, r in enumerate(sizes)]
    counts = matrix_of(rows)
    return counts, 350, sizes


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_the_triangle_decode_on_rows_around_every_boundary(torch_cuda, triangle, flags):
    torch = torch_cuda
    counts, nk, sizes = triangle
    want = nontrivial(counts, brute_force(counts, nk, flags))
    d = 1 if flags & DIAGONAL else -1
    assert want.cross == sum(r * (r + d) // 2 for r in sizes) > 1 << 17
    m, o = build_pair([b"aa", b"bb"], 1)
    plan = m.plan(0)
    mat = _matrix(torch, tallied_of(counts))
    check(plan.cooccur_matrix(mat, flags, n_keywords=nk), want, ("triangle", flags))
    plan.status()
    # the exact cross room, one slot more (a sentinel behind the pairs), and a row_limit between the sizes
    for room in (want.cross, want.cross + 1):
        check(plan.cooccur_matrix(mat, flags, n_keywords=nk, cross_capacity=room), want, ("triangle, room", flags, room))
    limited = brute_force(counts, nk, flags, 128)
    assert limited.skipped == 5 and 0 < limited.cross < want.cross
    check(plan.cooccur_matrix(mat, flags, 128, n_keywords=nk), limited, ("triangle, row_limit 128", flags))
    plan.status()


def test_one_wide_row_and_a_pair_every_text_holds(torch_cuda):
    """a row of 2,049 entries: 2.1 M pairs, every one once (the expected matrix is written down with numpy); and 5,000
    texts that all hold keywords 1 and 3, every third keyword 2 as well: runs as long as the batch"""
    torch = torch_cuda
    m, o = build_pair([b"aa", b"bb"], 1)
    plan = m.plan(0)
    r, nk = 2049, 2100
    ids = np.arange(3, 3 + r, dtype=np.uint32)
    counts = (np.array([0, 0, r], np.uint64), ids, np.ones(r, np.uint64))
    for flags in (0, DIAGONAL):
        lens = np.zeros(nk, np.int64)
        lens[3:3 + r] = np.arange(r, 0, -1) - (0 if flags else 1)
        col = np.concatenate([ids[i if flags else i + 1:] for i in range(r)])
        want = Expected(np.concatenate([[0], np.cumsum(lens)]), col, np.ones(col.size, np.uint64), col.size, 0, flags)
        assert want.nnz == r * (r + (1 if flags else -1)) // 2 > 1 << 21
        g = plan.cooccur_matrix(_matrix(torch, tallied_of(counts)), flags, n_keywords=nk)
        assert g.nnz == want.nnz and g.cross == want.cross
        assert np.array_equal(g.co_ptr.cpu().numpy().view(np.uint64), want.co_ptr)
        assert np.array_equal(g.co_col.cpu().numpy().view(np.uint32)[:g.nnz], want.co_col)
        assert bool((g.co_val[:g.nnz] == 1).all())
        plan.status()
    rows = [{1: 2, 3: 1 + t % 5, **({2: 7} if t % 3 == 0 else {})} for t in range(5000)]
    rows.insert(100, {})
    counts = matrix_of(rows)
    for flags in ALL_FLAGS:
        want = nontrivial(counts, brute_force(counts, 6, flags))
        assert want.entries()[(1, 3)] == (5000 if not flags & PRODUCT else sum(2 * (1 + t % 5) for t in range(5000)))
        check(plan.cooccur_matrix(_matrix(torch, tallied_of(counts)), flags, n_keywords=6), want, ("long runs", flags))
    plan.status()


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram, CSR, start-parallel, sparse walk, 8-byte symbols, comparator classes, a plan with a pending delta --
    through Plan.cooccur (four windows or more, one text over three whole windows) and Machine.cooccur, under a row_limit
    that keeps the pairs few; two keyword ids beyond the dictionary give the empty rows"""
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
    off = off[(off < window) | (off >= min(4 * window, text.size))]
    assert np.any(off[1:] == off[:-1]) and off[0] == 0 and off[-1] == text.size
    counts = expected(o, text, off)
    nk = o.nb_keywords + 2
    flags, limit = PRODUCT | DIAGONAL, 8
    want = nontrivial(counts, brute_force(counts, nk, flags, limit))
    records = int(counts[2].sum())
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([np.zeros(1, text.dtype), text]))[1:]
        assert dev.data_ptr() % 16 == 1
    else:
        dev = _dev(torch_cuda, text)
    g = plan.cooccur(dev, _dev(torch_cuda, off), flags, limit, n_keywords=nk, window=window, capacity=capacity, pair_capacity=records)
    print("entries %d, pair instances %d, skipped %d, total %d, largest window %d, partial pairs %d" % (g.nnz, g.cross, g.skipped, g.total, g.need, g.need_pairs))
    assert 0 < g.need <= capacity and g.total == records
    check(g, want, "%s Plan.cooccur" % name)
    plan.status()
    got = m.cooccur(_texts(text, off), flags, limit, n_keywords=nk)
    check(got, want, "%s Machine.cooccur" % name)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    plan.status()


def test_a_matrix_of_the_callers_own(torch_cuda):
    """counts near 2^64 wrap under PRODUCT as Python says; a d_col >= n_keywords loses every pair it is a member of, raises the
    plan's flag and is counted in cross all the same"""
    torch = torch_cuda
    rows = [{0: 1 << 63, 1: (1 << 64) - 1, 2: (1 << 63) + 1}, {}, {0: (1 << 64) - 1, 1: (1 << 64) - 1}, {1: 1 << 63, 2: 1 << 63, 3: 3}, {0: 3, 1: 5, 2: 7},
            {4: 1 << 32, 5: 1 << 32}]
    counts = matrix_of(rows)
    m, o = build_pair([b"aa", b"bb", b"cc"], 1)
    plan = m.plan(0)
    for flags in ALL_FLAGS:
        want = nontrivial(counts, brute_force(counts, 7, flags))
        if flags & PRODUCT:
            assert want.entries()[(4, 5)] == 0 and max(want.entries().values()) > 1 << 63
        check(plan.cooccur_matrix(_matrix(torch, tallied_of(counts)), flags, n_keywords=7), want, ("a caller's matrix", flags))
    plan.status()
    for flags in (0, PRODUCT | DIAGONAL):
        fresh = m.plan(0)
        bad = (counts[0], counts[1].copy(), counts[2])
        assert bad[1][7] == 3 and bad[0][3] == 5 and bad[0][4] == 8
        bad[1][7] = 9                                                      # text 3: {1, 2, 9}
        less = matrix_of([rows[0], {}, rows[2], {1: 1 << 63, 2: 1 << 63}, rows[4], rows[5]])
        want = brute_force(less, 7, flags)
        g = fresh.cooccur_matrix(_matrix(torch, tallied_of(bad)), flags, n_keywords=7)
        check(g, want, ("a col that is no keyword", flags), counts=False)
        assert g.cross == brute_force(counts, 7, flags).cross > want.cross
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7


class _Raw:
    """every output of the three device calls in an array of guard values (bytes of 0x5A) with 8 guard entries on either
    side of what the call may write"""

    def __init__(self, torch, n_keywords, room):
        def guard(n, dtype):
            return torch.full((n + 16,), GUARD32 if dtype == torch.int32 else GUARD64, dtype=dtype, device="cuda")
        self.co_ptr, self.co_col, self.co_val = guard(n_keywords + 1, torch.int64), guard(room, torch.int32), guard(room, torch.int64)
        self.res = torch.full((6,), 77, dtype=torch.int64, device="cuda")   # nnz, cross, skipped, total, need, need_pairs

    def p(self, name):
        a = getattr(self, name)
        return a.data_ptr() + 8 * a.element_size()

    def r(self, i):
        return self.res.data_ptr() + 8 * i

    def host(self, name):
        """(the part the call may write, whether the guards around it stand)"""
        a = getattr(self, name).cpu().numpy()
        g = GUARD32 if a.itemsize == 4 else GUARD64
        return a[8:-8], bool(np.all(a[:8] == g) and np.all(a[-8:] == g))

    def untouched(self, *names):
        for name in names:
            a, ok = self.host(name)
            assert ok and np.all(a == (GUARD32 if a.itemsize == 4 else GUARD64)), name

    def guards_stand(self):
        for name in ("co_ptr", "co_col", "co_val"):
            assert self.host(name)[1], name


def _raw_matrix(torch, plan, mat, n_texts, nk, flags, limit, cross_cap, out_cap, room, fill=True):
    """acm_gpu_cooccur_matrix_device into guarded arrays, the entries with `room` slots; (rc, res = [nnz, cross, skipped, ...], the _Raw)"""
    L = acm.lib()
    r = _Raw(torch, nk, room)
    tb = L.acm_gpu_cooccur_matrix_tmp_bytes(plan.h, n_texts, nk, cross_cap)
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_cooccur_matrix_device(plan.h, mat.row_ptr.data_ptr(), mat.col.data_ptr(), mat.val.data_ptr(), n_texts, nk, flags, limit, cross_cap,
                                         r.p("co_ptr"), r.p("co_col") if fill else None, r.p("co_val") if fill else None, out_cap, r.r(0), r.r(1), r.r(2),
                                         tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    return rc, r.res.cpu().tolist(), r


def _raw_cooccur(torch, plan, dev, d_off, n_texts, window, capacity, pair_capacity, flags, limit, cross_cap, out_cap, room):
    """acm_gpu_cooccur_device into guarded arrays; (rc, res = [nnz, cross, skipped, total, need, need_pairs], the _Raw)"""
    L = acm.lib()
    n = dev.numel()
    r = _Raw(torch, K, room)
    tb = L.acm_gpu_cooccur_tmp_bytes(plan.h, window, capacity, pair_capacity, n, n_texts, K, cross_cap)
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_cooccur_device(plan.h, dev.data_ptr(), n, d_off.data_ptr(), n_texts, window, capacity, pair_capacity, K, flags, limit, cross_cap,
                                  r.p("co_ptr"), r.p("co_col"), r.p("co_val"), out_cap, r.r(0), r.r(1), r.r(2), r.r(3), r.r(4), r.r(5), tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    return rc, r.res.cpu().tolist(), r


@pytest.mark.parametrize("flags", [0, PRODUCT | DIAGONAL])
def test_rooms_one_too_small_and_guards(torch_cuda, example, flags):
    torch = torch_cuda
    m, plan, text, off, counts = example
    want = brute_force(counts, K, flags, 3)
    mat = _matrix(torch, tallied_of(counts))
    n, cross = want.nnz, want.cross
    # one slot too little cross room: the need, *d_nnz = 0, skipped valid, nothing else written
    rc, res, r = _raw_matrix(torch, plan, mat, N, K, flags, 3, cross - 1, n, n)
    assert rc == 0 and res[:3] == [0, cross, 1]
    r.untouched("co_ptr", "co_col", "co_val")
    # one entry too little output room: the need, co_ptr complete, no byte outside the rooms
    rc, res, r = _raw_matrix(torch, plan, mat, N, K, flags, 3, cross, n - 1, n - 1)
    assert rc == 0 and res[:3] == [n, cross, 1]
    r.guards_stand()
    assert np.array_equal(r.host("co_ptr")[0].view(np.uint64), want.co_ptr)
    # exactly the rooms: the result, the guards around it stay
    rc, res, r = _raw_matrix(torch, plan, mat, N, K, flags, 3, cross, n, n)
    assert rc == 0 and res[:3] == [n, cross, 1]
    r.guards_stand()
    assert np.array_equal(r.host("co_ptr")[0].view(np.uint64), want.co_ptr) and np.array_equal(r.host("co_col")[0].view(np.uint32), want.co_col)
    assert np.array_equal(r.host("co_val")[0].view(np.uint64), want.co_val)
    # the count-only call: NULL entries, no room; the cross room is needed all the same
    rc, res, r = _raw_matrix(torch, plan, mat, N, K, flags, 3, cross, 0, n, fill=False)
    assert rc == 0 and res[:3] == [n, cross, 1]
    r.untouched("co_col", "co_val")
    assert np.array_equal(r.host("co_ptr")[0].view(np.uint64), want.co_ptr)
    rc, res, r = _raw_matrix(torch, plan, mat, N, K, flags, 3, 0, 0, n, fill=False)
    assert rc == 0 and res[:3] == [0, cross, 1]
    r.untouched("co_ptr")
    plan.status()
    # a matrix without a pair and no cross room at all: the empty result
    lone = _matrix(torch, tallied_of(matrix_of([{1: 4}, {}, {3: 1}])))
    rc, res, r = _raw_matrix(torch, plan, lone, 3, K, flags & PRODUCT, 0, 0, 4, 4)
    assert rc == 0 and res[:3] == [0, 0, 0] and r.host("co_ptr")[0].tolist() == [0] * (K + 1)
    r.untouched("co_col", "co_val")
    # Plan.cooccur_matrix with a cross room that is too small raises with the need; with an output room too small says so in nnz
    with pytest.raises(binding.ACMError) as e:
        plan.cooccur_matrix(mat, flags, 3, cross_capacity=cross - 1)
    assert e.value.code == binding.ACM_GPU_E_OVERFLOW and e.value.need == cross
    g = plan.cooccur_matrix(mat, flags, 3, out_capacity=n - 1)
    assert g.nnz == n > g.out_capacity and np.array_equal(g.co_ptr.cpu().numpy().view(np.uint64), want.co_ptr)
    # the host call: an overflow that leaves the entries alone
    ptr, small, val = np.zeros(K + 1, np.uint64), np.full(n - 1, GUARD32, np.uint32), np.full(n - 1, GUARD64, np.uint64)
    found, crossed, skipped, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = acm.lib().acm_gpu_cooccur_host(plan.h, text.ctypes.data, off.ctypes.data, N, K, flags, 3, ptr.ctypes.data, small.ctypes.data, val.ctypes.data, n - 1,
                                        C.byref(found), C.byref(crossed), C.byref(skipped), C.byref(total))
    assert rc == binding.ACM_GPU_E_OVERFLOW and (found.value, crossed.value, skipped.value, total.value) == (n, cross, 1, int(counts[2].sum()))
    assert np.array_equal(ptr, want.co_ptr) and np.all(small == GUARD32) and np.all(val == GUARD64)
    rc = acm.lib().acm_gpu_cooccur_host(plan.h, text.ctypes.data, off.ctypes.data, N, K, flags, 3, ptr.ctypes.data, None, None, 0, C.byref(found), None,
                                        None, None)
    assert rc == 0 and found.value == n and np.array_equal(ptr, want.co_ptr)


def test_the_host_call_repeats_once_with_the_cross_room_the_device_reported(torch_cuda):
    """more pair instances than the first guess of acm_gpu_cooccur_host (64 Ki): 40 texts that hold 64 keywords each"""
    torch = torch_cuda
    kws = [bytes([65 + i // 26, 97 + i % 26]) for i in range(64)]
    m, o = build_pair(kws, 1)
    texts = [b".".join(kws[(t + i) % 64] for i in range(64 - t % 3)) for t in range(40)]
    text, off = np.frombuffer(b"".join(texts), np.uint8), offsets_of(texts)
    counts = expected(o, text, off)
    want = nontrivial(counts, brute_force(counts, 66, DIAGONAL))
    assert want.cross > 1 << 16
    plan = m.plan(0)
    check(plan.cooccur_host(text, off, DIAGONAL, n_keywords=66), want, "Plan.cooccur_host, two cross rooms")
    check(plan.cooccur(_dev(torch, text), _dev(torch, off), DIAGONAL, n_keywords=66), want, "Plan.cooccur, two cross rooms")
    plan.status()


def test_arguments(torch_cuda, example):
    torch = torch_cuda
    m, plan, text, off, counts = example
    dev, d_off = _dev(torch, text), _dev(torch, off)
    L = acm.lib()
    tmp = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, dtype=torch.int64, device="cuda")
    p = out.data_ptr()
    E = binding.ACM_GPU_E_ARG
    good = dict(ptr=p, col=p + 256, val=p + 512, cap=4, nnz=p + 1024, cross=p + 1032, skipped=p + 1040, nt=N, nk=K, flags=0, room=64)
    for change in (dict(col=None), dict(val=None), dict(ptr=None), dict(nnz=None), dict(cross=None), dict(skipped=None), dict(nt=1 << 31), dict(nk=K - 1),
                   dict(nk=1 << 32), dict(flags=4), dict(flags=1 << 31), dict(cap=1 << 31), dict(room=1 << 31), dict(col=None, val=None)):
        a = dict(good, **change)
        assert L.acm_gpu_cooccur_device(plan.h, dev.data_ptr(), dev.numel(), d_off.data_ptr(), a["nt"], 16, 64, 64, a["nk"], a["flags"], 0, a["room"], a["ptr"],
                                        a["col"], a["val"], a["cap"], a["nnz"], a["cross"], a["skipped"], p + 1048, p + 1056, p + 1064, tmp.data_ptr(),
                                        tmp.numel(), None) == E, change
        assert L.acm_gpu_cooccur_matrix_device(plan.h, p + 1100, p + 1200, p + 1300, a["nt"], a["nk"], a["flags"], 0, a["room"], a["ptr"], a["col"], a["val"],
                                               a["cap"], a["nnz"], a["cross"], a["skipped"], tmp.data_ptr(), tmp.numel(), None) == E, change
    assert L.acm_gpu_cooccur_matrix_tmp_bytes(plan.h, 1 << 31, K, 8) == 0 and L.acm_gpu_cooccur_matrix_tmp_bytes(plan.h, N, 1 << 32, 8) == 0
    assert L.acm_gpu_cooccur_matrix_tmp_bytes(plan.h, N, K, 1 << 31) == 0 and L.acm_gpu_cooccur_tmp_bytes(plan.h, 16, 0, 8, text.size, N, K, 8) == 0
    assert L.acm_gpu_cooccur_tmp_bytes(plan.h, 16, 64, 64, text.size, N, K, 1 << 31) == 0 and L.acm_gpu_cooccur_add_tmp_bytes(plan.h, K, 1 << 31) == 0
    assert L.acm_gpu_cooccur_add_tmp_bytes(plan.h, 1 << 32, 8) == 0
    assert L.acm_gpu_cooccur_matrix_tmp_bytes(plan.h, N, K - 1, 8) == 0 and L.acm_gpu_cooccur_tmp_bytes(plan.h, 16, 64, 64, text.size, N, K - 1, 8) == 0
    assert L.acm_gpu_cooccur_matrix_tmp_bytes(plan.h, N, K, 8) > 0 and L.acm_gpu_cooccur_tmp_bytes(plan.h, 16, 64, 64, text.size, N, K, 8) > 0
    assert L.acm_gpu_cooccur_matrix_device(plan.h, p + 1100, p + 1200, p + 1300, N, K, 0, 0, 64, p, p + 256, p + 512, 4, p + 1024, p + 1032, p + 1040,
                                           tmp.data_ptr(), 16, None) == E   # scratch that is too small
    with pytest.raises(binding.ACMError):
        plan.cooccur(dev, d_off, flags=4)
    # no text at all: every output is set
    raw = _Raw(torch, K, 4)
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.acm_gpu_cooccur_matrix_device(plan.h, zero.data_ptr(), None, None, 0, K, 3, 0, 0, raw.p("co_ptr"), raw.p("co_col"), raw.p("co_val"), 4, raw.r(0),
                                           raw.r(1), raw.r(2), None, 0, None) == 0
    torch.cuda.synchronize()
    assert raw.res.cpu().tolist()[:3] == [0, 0, 0] and raw.host("co_ptr")[0].tolist() == [0] * (K + 1)
    raw.guards_stand()
    g = plan.cooccur(dev[:0], zero, DIAGONAL)
    assert (g.nnz, g.cross, g.skipped) == (0, 0, 0) and g.co_ptr.cpu().tolist() == [0] * (K + 1)


def test_a_row_ptr_that_decreases_writes_nothing(torch_cuda):
    torch = torch_cuda
    m, o = build_pair([b"he", b"she"], 1)
    for what, bad in (("decreasing", [0, 2, 1, 3]), ("first", [1, 1, 2, 3])):
        fresh = m.plan(0)
        mat = _matrix(torch, binding.TalliedBatch(np.array(bad), np.array([0, 1, 1]), np.array([1, 1, 1]), 3, 0))
        rc, res, r = _raw_matrix(torch, fresh, mat, 3, 2, DIAGONAL, 0, 16, 16, 16)
        assert rc == 0, what
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        assert res[:3] == [0, 0, 77], what
        r.untouched("co_ptr", "co_col", "co_val")


def test_window_and_pair_overflow_pass_through(torch_cuda, example):
    """what tally_batch reports comes through: *d_nnz = *d_cross = 0, nothing else written; the repeat with the reported rooms is whole"""
    torch = torch_cuda
    m, plan, text, off, counts = example
    want = brute_force(counts, K, DIAGONAL)
    dev, d_off = _dev(torch, text), _dev(torch, off)
    n, records = want.nnz, int(counts[2].sum())
    rc, res, r = _raw_cooccur(torch, plan, dev, d_off, N, 16, 64, records, DIAGONAL, 0, want.cross, n, n)
    assert rc == 0 and res[:4] == [n, want.cross, 0, records] and 1 < res[4] <= 64
    assert np.array_equal(r.host("co_col")[0].view(np.uint32), want.co_col) and np.array_equal(r.host("co_val")[0].view(np.uint64), want.co_val)
    r.guards_stand()
    need = res[4]
    rc, res, r = _raw_cooccur(torch, plan, dev, d_off, N, 16, need - 1, records, DIAGONAL, 0, want.cross, n, n)   # a window with more records than room
    assert rc == 0 and res[0] == 0 and res[1] == 0 and res[2] == 77 and res[3] == 0 and res[4] >= need
    r.untouched("co_ptr", "co_col", "co_val")
    plan.status()
    rc, res, r = _raw_cooccur(torch, plan, dev, d_off, N, 16, 64, 1, DIAGONAL, 0, want.cross, n, n)               # more partial pairs than room
    assert rc == 0 and res[0] == 0 and res[1] == 0 and res[2] == 77 and res[5] == records
    r.untouched("co_ptr", "co_col", "co_val")
    plan.status()
    g = plan.cooccur(dev, d_off, DIAGONAL, window=16, capacity=res[4], pair_capacity=res[5])
    check(g, want, "the repeat")
    plan.status()
    # offsets that break the contract: nothing written, the flag raised
    fresh = m.plan(0)
    broken = off.copy()
    broken[3], broken[4] = off[4] + 1, off[3]
    rc, res, r = _raw_cooccur(torch, fresh, dev, _dev(torch, broken), N, 16, 64, records, DIAGONAL, 0, want.cross, n, n)
    assert rc == 0 and res[0] == 0 and res[1] == 0
    r.untouched("co_ptr", "co_col", "co_val")
    with pytest.raises(binding.ACMError):
        fresh.status()


def _add_both(torch, plan, a, b, what):
    """ADD of two Expected on the device, held against the host function's answer and returned"""
    host = binding.cooccur_add(cooccurred_of(a), cooccurred_of(b))
    got = plan.cooccur_add(_device_matrix(torch, a), _device_matrix(torch, b))
    assert got.nnz == host.nnz and np.array_equal(got.co_ptr.cpu().numpy().view(np.uint64), host.co_ptr), what
    assert np.array_equal(got.co_col.cpu().numpy().view(np.uint32)[:got.nnz], host.co_col), what
    assert np.array_equal(got.co_val.cpu().numpy().view(np.uint64)[:got.nnz], host.co_val), what
    plan.status()
    return got


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_add_on_the_device(torch_cuda, example, triangle, flags):
    torch = torch_cuda
    m, plan, text, off, counts = example
    whole = nontrivial(counts, brute_force(counts, K, flags))
    # the halves of the example; A over four keywords (the dictionary grew)
    a, b = brute_force(cut_rows(counts, 0, 7), K, flags), brute_force(cut_rows(counts, 7, N), K, flags)
    assert a.nnz > 0 and b.nnz > 0 and whole.nnz < a.nnz + b.nnz
    check(_add_both(torch, plan, a, b, "halves"), whole, "halves")
    check(_add_both(torch, plan, b, a, "halves, the other way round"), whole, "halves, the other way round")
    a4 = brute_force(cut_rows(counts, 0, 7), 4, flags)
    check(_add_both(torch, plan, a4, b, "grown"), whole, "a dictionary that grew")
    # the triangle matrix cut in two: both halves by the device's own passes, then their sum
    tcounts, nk, sizes = triangle
    twhole = brute_force(tcounts, nk, flags)
    halves = [plan.cooccur_matrix(_matrix(torch, tallied_of(cut_rows(tcounts, lo, hi))), flags, n_keywords=nk) for lo, hi in ((0, 12), (12, len(sizes)))]
    assert halves[0].nnz + halves[1].nnz > twhole.nnz > max(halves[0].nnz, halves[1].nnz)
    check(plan.cooccur_add(halves[0], halves[1]), twhole, ("the triangle cut at 12", flags))
    plan.status()


def test_add_wraps_and_its_rooms_and_violations(torch_cuda, example):
    torch = torch_cuda
    m, plan, text, off, counts = example
    wa = brute_force(matrix_of([{0: 1 << 63, 1: 3}]), K, PRODUCT | DIAGONAL)
    wb = brute_force(matrix_of([{0: (1 << 63) + 1, 1: 5}, {1: 1 << 32}]), K, PRODUCT | DIAGONAL)
    wrapped = add_expected(wa, wb)
    assert wrapped.entries()[(0, 1)] == (3 * (1 << 63) + 5 * ((1 << 63) + 1)) & MASK and wrapped.entries()[(0, 0)] == 1
    check(_add_both(torch, plan, wa, wb, "wrap"), wrapped, "wrap")
    flags = DIAGONAL
    whole = brute_force(counts, K, flags)
    a, b = brute_force(cut_rows(counts, 0, 7), K, flags), brute_force(cut_rows(counts, 7, N), K, flags)
    A, B = _device_matrix(torch, a), _device_matrix(torch, b)
    n, both = whole.nnz, a.nnz + b.nnz
    L = acm.lib()

    def raw(plan, A, B, cross_cap, cap, room, fill=True, n_a=K, n_b=K):
        r = _Raw(torch, K, room)
        tb = L.acm_gpu_cooccur_add_tmp_bytes(plan.h, n_b, cross_cap)
        tmp = torch.empty(max(tb, 16), dtype=torch.uint8, device="cuda")
        rc = L.acm_gpu_cooccur_add_device(plan.h, A.co_ptr.data_ptr(), A.co_col.data_ptr(), A.co_val.data_ptr(), n_a, B.co_ptr.data_ptr(), B.co_col.data_ptr(),
                                          B.co_val.data_ptr(), n_b, cross_cap, r.p("co_ptr"), r.p("co_col") if fill else None, r.p("co_val") if fill else None,
                                          cap, r.r(0), r.r(1), tmp.data_ptr(), tb, None)
        torch.cuda.synchronize()
        return rc, r.res.cpu().tolist()[:2], r
    rc, res, r = raw(plan, A, B, both - 1, n, n)                          # one slot too little cross room
    assert rc == 0 and res == [0, both]
    r.untouched("co_ptr", "co_col", "co_val")
    rc, res, r = raw(plan, A, B, both, n - 1, n - 1)                      # one entry too little output room
    assert rc == 0 and res == [n, both] and np.array_equal(r.host("co_ptr")[0].view(np.uint64), whole.co_ptr)
    r.guards_stand()
    rc, res, r = raw(plan, A, B, both, n, n)
    assert rc == 0 and res == [n, both] and np.array_equal(r.host("co_col")[0].view(np.uint32), whole.co_col)
    assert np.array_equal(r.host("co_val")[0].view(np.uint64), whole.co_val)
    r.guards_stand()
    rc, res, r = raw(plan, A, B, both, 0, n, fill=False)
    assert rc == 0 and res == [n, both] and np.array_equal(r.host("co_ptr")[0].view(np.uint64), whole.co_ptr)
    r.untouched("co_col", "co_val")
    plan.status()
    assert raw(plan, A, B, both, n, n, n_a=K, n_b=K - 1)[0] == binding.ACM_GPU_E_ARG
    with pytest.raises(binding.ACMError) as e:
        plan.cooccur_add(A, B, cross_capacity=both - 1)
    assert e.value.code == binding.ACM_GPU_E_OVERFLOW and e.value.need == both
    # the violations: the flag is raised, *d_out_nnz = *d_cross = 0, nothing else is written
    down = binding.Cooccurred(_dev(torch, np.array([0, 3, 2, 5, 7, 7], np.uint64)), A.co_col, A.co_val, 7)
    first = binding.Cooccurred(_dev(torch, np.array([1, 3, 5, 6, 7, 7], np.uint64)), A.co_col, A.co_val, 7)
    for what, (x, y) in (("a pointer array that decreases", (down, B)), ("B's decreases", (A, down)), ("A's begins with 1", (first, B))):
        fresh = m.plan(0)
        rc, res, r = raw(fresh, x, y, both, n, n)
        assert rc == 0 and res == [0, 0], what
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        r.untouched("co_ptr", "co_col", "co_val")
    # an entry whose col is no keyword of B's is dropped and raises the flag
    fresh = m.plan(0)
    high = a.co_col.copy()
    assert (int(high[-1]), int(a.co_ptr[3]), int(a.co_ptr[4])) == (3, a.nnz - 1, a.nnz)       # the last entry is (3, 3)
    high[-1] = K
    less = Expected(np.concatenate([a.co_ptr[:4], [a.nnz - 1, a.nnz - 1]]), a.co_col[:-1], a.co_val[:-1], 0, 0, flags)
    bad = binding.Cooccurred(A.co_ptr, _dev(torch, high), A.co_val, a.nnz)
    got = fresh.cooccur_add(bad, B)
    check(got, add_expected(less, b), "a col that is no keyword", counts=False)
    with pytest.raises(binding.ACMError) as e:
        fresh.status()
    assert e.value.code == -7
