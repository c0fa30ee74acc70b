"""The inverted index of a batch on the GPU (acm_gpu_index_*, acm_index; csrc/dev_index.h).  The expected index is
always the brute-force transposition of the ORACLE's count matrix (tests/index_cases.py over
tests/tally_batch_cases.expected), never of the library's own counts; every workload first shows from the oracle alone
that it cannot pass trivially, and where a form is named the call's d_forms show that it ran."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import offsets_of, random_cuts
from tests.cases import build_pair
from tests.index_cases import (EXAMPLE_KEYWORDS, EXAMPLE_NNZ, EXAMPLE_PTR, EXAMPLE_TEXTS, EXAMPLE_TOTAL, brute_force, check, concat_expected, cut_rows,
                               forms_of, indexed_of, nontrivial, tallied_of)
from tests.tally_batch_cases import expected
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind
from tests.test_score_gpu import _dev, _matrix, _texts

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
K = len(EXAMPLE_KEYWORDS)
N = len(EXAMPLE_TEXTS)
TOP_BASE = (1 << 32) - N
DEFAULT_LIST = 1024


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
    whole = brute_force(counts, K)
    assert whole.post_ptr.tolist() == EXAMPLE_PTR and whole.nnz == EXAMPLE_NNZ and whole.total == EXAMPLE_TOTAL
    plan = m.plan(0)
    assert plan.info.kernel == 1, plan.describe()
    return m, plan, text, off, counts


def _device_index(torch, e):
    """an Expected as an Indexed of device tensors (the input of a CONCAT on the device)"""
    def some(a):
        return _dev(torch, a) if a.size else torch.zeros(1, dtype={4: torch.int32, 8: torch.int64}[a.itemsize], device="cuda")
    return binding.Indexed(_dev(torch, e.post_ptr), some(e.post_text), some(e.post_count), e.nnz, e.total, e.text_base)


@pytest.mark.parametrize("base", [0, TOP_BASE])
@pytest.mark.parametrize("longest", [None, 1, 4])
def test_the_example_through_the_four_routes(torch_cuda, monkeypatch, example, longest, base):
    """the worked example of the header in windows of 16 symbols.  With ACM_GPU_INDEX_LIST = 1 the four lists go through
    the wide form, with 4 `he` (5) and `s` (7) do while `she` (2) and `hers` (3) are sorted by a wave"""
    torch = torch_cuda
    m, plan, text, off, counts = example
    if longest:
        monkeypatch.setenv("ACM_GPU_INDEX_LIST", str(longest))
    forms = {None: (4, 0), 1: (0, 4), 4: (2, 2)}[longest]
    want = nontrivial(counts, brute_force(counts, K, base), longest or DEFAULT_LIST, *forms)
    records = int(counts[2].sum())
    assert records == EXAMPLE_TOTAL
    dev, d_off = _dev(torch, text), _dev(torch, off)
    g = plan.index_matrix(_matrix(torch, tallied_of(counts)), text_base=base)
    check(g, want, ("Plan.index_matrix", longest, base), total=False)
    assert g.forms == forms, g.forms
    plan.status()
    g = plan.index(dev, d_off, text_base=base, window=16, capacity=64, pair_capacity=records)
    assert 0 < g.need <= 64
    check(g, want, ("Plan.index", longest, base))
    assert g.forms == forms, g.forms
    dense = g.to_sparse_csr(N).to_dense().cpu().numpy()
    assert np.array_equal(dense, np.array([[dict(zip((want.post_text[int(a):int(b)].astype(np.int64) - base).tolist(), want.post_count[int(a):int(b)].tolist())).get(t, 0)
                                            for t in range(N)] for a, b in zip(want.post_ptr[:-1], want.post_ptr[1:])]))
    assert [x.cpu().tolist() for x in g.postings(1)] == [[x - (1 << 32) if x >= 1 << 31 else x for x in (base + 3, base + 11)], [1, 2]]
    plan.status()
    check(plan.index_host(text, off, text_base=base), want, ("Plan.index_host", longest, base))
    plan.status()
    got = m.index(EXAMPLE_TEXTS, text_base=base)
    check(got, want, ("Machine.index", longest, base))
    assert m.scan_path == PATH_GPU
    # more keywords than the plan has: empty lists behind
    check(plan.index(dev, d_off, n_keywords=K + 3, text_base=base, window=16, capacity=64), brute_force(counts, K + 3, base), ("K + 3", longest, base))
    plan.status()


@pytest.fixture(scope="module")
def long_list():
    """5,000 texts of one to three symbols that all hold `s` (every third is `she`, which holds `he` and `she` too), an
    empty text behind every seventh: (machine, text, offsets, the oracle's count matrix, the texts), made once"""
    m, o = build_pair(EXAMPLE_KEYWORDS, 1)
    texts = []
    for i in range(5000):
        texts.append(b"she" if i % 3 == 0 else (b"s", b"us", b"ss", b"s.")[(i // 3) % 4])
        if i % 7 == 6:
            texts.append(b"")
    text, off = np.frombuffer(b"".join(texts), np.uint8), offsets_of(texts)
    counts = expected(o, text, off)
    want = brute_force(counts, K)
    assert want.df.tolist() == [1667, 1667, 0, 5000, 0] and len(texts) == 5714 and int(counts[2].max()) == 2
    return m, text, off, counts, texts


@pytest.mark.parametrize("longest", [None, 64, 4096])
def test_a_list_longer_than_the_fast_form_can_ever_take(torch_cuda, monkeypatch, long_list, longest):
    """df (s) = 5,000 > 4,096: the wide form whatever the environment says; `he` and `she` (1,667) go wide at 1,024 and at
    64 and are sorted by one block at 4,096 (64 KiB of LDS)"""
    torch = torch_cuda
    m, text, off, counts, texts = long_list
    if longest:
        monkeypatch.setenv("ACM_GPU_INDEX_LIST", str(longest))
    forms = (2, 1) if longest == 4096 else (0, 3)
    want = nontrivial(counts, brute_force(counts, K, 7), longest or DEFAULT_LIST, *forms)
    plan = m.plan(0)
    records = int(counts[2].sum())
    g = plan.index(_dev(torch, text), _dev(torch, off), text_base=7, window=4096, capacity=1 << 14, pair_capacity=1 << 14)
    check(g, want, ("long list, Plan.index", longest))
    assert g.forms == forms and g.total == records
    plan.status()
    g = plan.index_matrix(_matrix(torch, tallied_of(counts)), text_base=7, post_capacity=want.nnz + 5)
    check(g, want, ("long list, Plan.index_matrix", longest), total=False)
    assert g.forms == forms
    plan.status()


@pytest.mark.parametrize("longest", [None, 100])
def test_lists_of_every_tier(torch_cuda, monkeypatch, longest):
    """a caller's matrix of 1,500 texts over 40 keywords with lists of 0, 1, 2, 63 .. 65, 255 .. 257, 1,023 .. 1,025 and
    1,500 entries: both sides of the one-wave tier (256), of the one-block tier (ACM_GPU_INDEX_LIST) and of the wide form"""
    torch = torch_cuda
    sizes = [0, 1, 2, 3, 63, 64, 65, 99, 100, 101, 255, 256, 257, 300, 1023, 1024, 1025, 1500, 0, 7]
    rng = np.random.default_rng(5)
    n_texts, nk = 1500, len(sizes)
    rows = [[] for _ in range(n_texts)]
    for k, df in enumerate(sizes):
        for t in np.sort(rng.choice(n_texts, size=df, replace=False)).tolist():
            rows[t].append((k, int(rng.integers(1, 1 << 50))))
    row_ptr, col, val = [0], [], []
    for r in rows:
        col += [k for k, _ in r]
        val += [v for _, v in r]
        row_ptr.append(len(col))
    counts = (np.array(row_ptr, np.uint64), np.array(col, np.uint32), np.array(val, np.uint64))
    if longest:
        monkeypatch.setenv("ACM_GPU_INDEX_LIST", str(longest))
    top = longest or DEFAULT_LIST
    forms = (sum(1 for s in sizes if 1 <= s <= top), sum(1 for s in sizes if s > top))
    want = nontrivial(counts, brute_force(counts, nk), top, *forms)
    assert forms[0] > 0 and forms[1] > 0
    m, o = build_pair([b"aa", b"bb"], 1)
    plan = m.plan(0)
    g = plan.index_matrix(_matrix(torch, tallied_of(counts)), n_keywords=nk)
    check(g, want, ("tiers", longest), total=False)
    assert g.forms == forms
    plan.status()


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram, CSR, start-parallel, sparse walk, 8-byte symbols, comparator classes, a plan with a pending delta --
    through Plan.index (four windows or more, one text over three whole windows) and Machine.index: many short lists;
    two keyword ids beyond the dictionary give the empty lists"""
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
    want = nontrivial(counts, brute_force(counts, nk, 100))
    print("lists by either form: %s" % (forms_of(want, DEFAULT_LIST),))
    records = int(counts[2].sum())
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([np.zeros(1, text.dtype), text]))[1:]
        assert dev.data_ptr() % 16 == 1
    else:
        dev = _dev(torch_cuda, text)
    g = plan.index(dev, _dev(torch_cuda, off), n_keywords=nk, text_base=100, window=window, capacity=capacity, pair_capacity=records,
                   post_capacity=want.nnz)
    print("entries %d, total %d, largest window %d, partial pairs %d" % (g.nnz, g.total, g.need, g.need_pairs))
    assert 0 < g.need <= capacity and g.total == records
    check(g, want, "%s Plan.index" % name)
    assert g.forms == forms_of(want, DEFAULT_LIST)
    plan.status()
    got = m.index(_texts(text, off), n_keywords=nk, text_base=100)
    check(got, want, "%s Machine.index" % name)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    plan.status()


def test_a_matrix_of_the_callers_own(torch_cuda):
    """counts above 2^32 come through whole; a d_col >= n_keywords is not counted and raises the plan's flag"""
    torch = torch_cuda
    rows = [{0: 1 << 40, 1: 1 << 63}, {}, {1: (1 << 63) + 3, 2: 5}, {0: (1 << 64) - 1, 1: 1 << 62, 2: 1 << 40}]
    row_ptr, col, val = [0], [], []
    for row in rows:
        col += sorted(row)
        val += [row[k] for k in sorted(row)]
        row_ptr.append(len(col))
    counts = (np.array(row_ptr, np.uint64), np.array(col, np.uint32), np.array(val, np.uint64))
    want = nontrivial(counts, brute_force(counts, 4, 9))
    assert int(want.post_count.max()) > 1 << 32
    m, o = build_pair([b"aa", b"bb", b"cc"], 1)
    plan = m.plan(0)
    g = plan.index_matrix(_matrix(torch, tallied_of(counts)), n_keywords=4, text_base=9)
    check(g, want, "a caller's matrix", total=False)
    plan.status()
    for longest in (None, 1):                                              # (the skip is the count pass's: either form behind it)
        fresh = m.plan(0)
        bad = (counts[0], counts[1].copy(), counts[2])
        bad[1][3] = 7                                                      # text 2: {1, 7}
        less = (np.array([0, 2, 2, 3, 6], np.uint64), np.delete(counts[1], 3), np.delete(counts[2], 3))
        with pytest.MonkeyPatch.context() as mp:
            if longest:
                mp.setenv("ACM_GPU_INDEX_LIST", str(longest))
            g = fresh.index_matrix(_matrix(torch, tallied_of(bad)), n_keywords=4, text_base=9)
        check(g, brute_force(less, 4, 9), ("a col that is no keyword", longest), total=False)
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7


class _Raw:
    """every output of the three device calls in an array of guard values (bytes of 0x5A) with 8 guard entries on either
    side of what the call may write"""

    def __init__(self, torch, n_keywords, room):
        def guard(n, dtype):
            return torch.full((n + 16,), GUARD32 if dtype == torch.int32 else GUARD64, dtype=dtype, device="cuda")
        self.post_ptr, self.post_text, self.post_count = guard(n_keywords + 1, torch.int64), guard(room, torch.int32), guard(room, torch.int64)
        self.forms = guard(2, torch.int64)
        self.res = torch.full((4,), 77, dtype=torch.int64, device="cuda")

    def p(self, name):
        a = getattr(self, name)
        return a.data_ptr() + 8 * a.element_size()

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
        for name in ("post_ptr", "post_text", "post_count", "forms"):
            assert self.host(name)[1], name


def _raw_index(torch, plan, dev, d_off, n_texts, window, capacity, pair_capacity, post_capacity, room, fill=True):
    """acm_gpu_index_device into guarded arrays, the lists with `room` entries; (rc, res = [nnz, total, need, need_pairs], the _Raw)"""
    L = acm.lib()
    n = dev.numel()
    r = _Raw(torch, K, room)
    tb = L.acm_gpu_index_tmp_bytes(plan.h, window, capacity, pair_capacity, n, n_texts, K, post_capacity)
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_index_device(plan.h, dev.data_ptr(), n, d_off.data_ptr(), n_texts, window, capacity, pair_capacity, K, 0, r.p("post_ptr"),
                                r.p("post_text") if fill else None, r.p("post_count") if fill else None, post_capacity, r.res.data_ptr(), r.p("forms"),
                                r.res.data_ptr() + 8, r.res.data_ptr() + 16, r.res.data_ptr() + 24, tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    return rc, r.res.cpu().tolist(), r


@pytest.mark.parametrize("longest", [None, 4])
def test_post_capacity_one_too_small_and_guards(torch_cuda, monkeypatch, example, longest):
    torch = torch_cuda
    m, plan, text, off, counts = example
    if longest:
        monkeypatch.setenv("ACM_GPU_INDEX_LIST", str(longest))
    want = brute_force(counts, K)
    dev, d_off = _dev(torch, text), _dev(torch, off)
    n, records = want.nnz, want.total
    # one entry too little room: the need, post_ptr complete (so df is known), no byte outside the rooms, no list put in order
    rc, res, r = _raw_index(torch, plan, dev, d_off, N, 16, 64, records, n - 1, n - 1)
    assert rc == 0 and res[0] == n and res[1] == records and 0 < res[2] <= 64
    r.guards_stand()
    assert np.array_equal(r.host("post_ptr")[0].view(np.uint64), want.post_ptr) and r.host("forms")[0].tolist() == [0, 0]
    # exactly the room: the result, the guards around it stay
    rc, res, r = _raw_index(torch, plan, dev, d_off, N, 16, 64, records, n, n)
    assert rc == 0 and res[0] == n
    r.guards_stand()
    assert np.array_equal(r.host("post_ptr")[0].view(np.uint64), want.post_ptr) and np.array_equal(r.host("post_text")[0].view(np.uint32), want.post_text)
    assert np.array_equal(r.host("post_count")[0].view(np.uint64), want.post_count)
    assert tuple(r.host("forms")[0].tolist()) == forms_of(want, longest or DEFAULT_LIST)
    plan.status()
    # the count-only call: NULL lists, no room
    rc, res, r = _raw_index(torch, plan, dev, d_off, N, 16, 64, records, 0, n, fill=False)
    assert rc == 0 and res[0] == n and res[1] == records
    r.untouched("post_text", "post_count")
    r.guards_stand()
    assert np.array_equal(r.host("post_ptr")[0].view(np.uint64), want.post_ptr) and r.host("forms")[0].tolist() == [0, 0]
    plan.status()
    # Plan.index with a room that is too small says so in nnz; df is there all the same
    g = plan.index(dev, d_off, window=16, capacity=64, pair_capacity=records, post_capacity=n - 1)
    assert g.nnz == n > g.post_capacity and g.df().cpu().tolist() == want.df.tolist()
    # the host call: an overflow that leaves the lists alone
    ptr, small, cnt, found, total = np.zeros(K + 1, np.uint64), np.full(n - 1, GUARD32, np.uint32), np.full(n - 1, GUARD64, np.uint64), C.c_uint64(0), C.c_uint64(0)
    rc = acm.lib().acm_gpu_index_host(plan.h, text.ctypes.data, off.ctypes.data, N, 0, ptr.ctypes.data, K, small.ctypes.data, cnt.ctypes.data, n - 1,
                                      C.byref(found), C.byref(total))
    assert rc == binding.ACM_GPU_E_OVERFLOW and found.value == n and total.value == records and np.array_equal(ptr, want.post_ptr)
    assert np.all(small == GUARD32) and np.all(cnt == GUARD64)
    rc = acm.lib().acm_gpu_index_host(plan.h, text.ctypes.data, off.ctypes.data, N, 0, ptr.ctypes.data, K, None, None, 0, C.byref(found), C.byref(total))
    assert rc == 0 and found.value == n and np.array_equal(ptr, want.post_ptr)
    # arguments
    L = acm.lib()
    tmp = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, dtype=torch.int64, device="cuda")
    p = out.data_ptr()
    for ptr_p, text_p, count_p, cap, nnz_p, nt, nk, base in ((p, None, p + 512, 4, p + 1024, N, K, 0), (p, p + 256, None, 4, p + 1024, N, K, 0),
                                                             (None, p + 256, p + 512, 4, p + 1024, N, K, 0), (p, p + 256, p + 512, 4, None, N, K, 0),
                                                             (p, p + 256, p + 512, 4, p + 1024, 1 << 31, K, 0), (p, p + 256, p + 512, 4, p + 1024, N, K - 1, 0),
                                                             (p, p + 256, p + 512, 4, p + 1024, N, 1 << 32, 0), (p, p + 256, p + 512, 4, p + 1024, N, K, TOP_BASE + 1),
                                                             (p, p + 256, p + 512, 1 << 31, p + 1024, N, K, 0), (p, None, None, 4, p + 1024, N, K, 0)):
        assert L.acm_gpu_index_device(plan.h, dev.data_ptr(), dev.numel(), d_off.data_ptr(), nt, 16, 64, 64, nk, base, ptr_p, text_p, count_p, cap, nnz_p, None,
                                      p + 1032, p + 1040, p + 1048, tmp.data_ptr(), tmp.numel(), None) == binding.ACM_GPU_E_ARG
        assert L.acm_gpu_index_matrix_device(plan.h, p + 1100, p + 1200, p + 1300, nt, nk, base, ptr_p, text_p, count_p, cap, nnz_p, None, tmp.data_ptr(),
                                             tmp.numel(), None) == binding.ACM_GPU_E_ARG
    assert L.acm_gpu_index_matrix_tmp_bytes(plan.h, 1 << 31, K, 8) == 0 and L.acm_gpu_index_tmp_bytes(plan.h, 16, 0, 8, text.size, N, K, 8) == 0
    assert L.acm_gpu_index_matrix_device(plan.h, p + 1100, p + 1200, p + 1300, N, K, 0, p, p + 256, p + 512, 4, p + 1024, None, tmp.data_ptr(), 16, None) == \
        binding.ACM_GPU_E_ARG                                              # scratch that is too small


def test_a_row_ptr_that_decreases_writes_nothing(torch_cuda):
    torch = torch_cuda
    m, o = build_pair([b"he", b"she"], 1)
    L = acm.lib()
    for what, bad in (("decreasing", [0, 2, 1, 3]), ("first", [1, 1, 2, 3])):
        fresh = m.plan(0)
        mat = _matrix(torch, binding.TalliedBatch(np.array(bad), np.array([0, 1, 1]), np.array([1, 1, 1]), 3, 0))
        r = _Raw(torch, 2, 16)
        tb = L.acm_gpu_index_matrix_tmp_bytes(fresh.h, 3, 2, 16)
        tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
        rc = L.acm_gpu_index_matrix_device(fresh.h, mat.row_ptr.data_ptr(), mat.col.data_ptr(), mat.val.data_ptr(), 3, 2, 0, r.p("post_ptr"), r.p("post_text"),
                                           r.p("post_count"), 16, r.res.data_ptr(), r.p("forms"), tmp.data_ptr(), tb, None)
        assert rc == 0, what
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        assert int(r.res[0].item()) == 0, what
        r.untouched("post_ptr", "post_text", "post_count", "forms")


def test_window_and_pair_overflow_pass_through(torch_cuda, example):
    """what tally_batch reports comes through: *d_nnz = 0, nothing else written; the repeat with the reported rooms is whole"""
    torch = torch_cuda
    m, plan, text, off, counts = example
    want = brute_force(counts, K)
    dev, d_off = _dev(torch, text), _dev(torch, off)
    n, records = want.nnz, want.total
    rc, res, r = _raw_index(torch, plan, dev, d_off, N, 16, 64, records, n, n)
    assert rc == 0 and res[0] == n and 1 < res[2] <= 64
    need = res[2]
    rc, res, r = _raw_index(torch, plan, dev, d_off, N, 16, need - 1, records, n, n)      # a window with more records than room
    assert rc == 0 and res[0] == 0 and res[1] == 0 and res[2] >= need > need - 1
    r.untouched("post_ptr", "post_text", "post_count", "forms")
    plan.status()
    rc, res, r = _raw_index(torch, plan, dev, d_off, N, 16, 64, 1, n, n)                  # more partial pairs than room
    assert rc == 0 and res[0] == 0 and res[1] == 0 and res[3] == records
    r.untouched("post_ptr", "post_text", "post_count", "forms")
    plan.status()
    g = plan.index(dev, d_off, window=16, capacity=res[2], pair_capacity=res[3])
    check(g, want, "the repeat")
    plan.status()


def _concat_both(torch, plan, a, b, what):
    """CONCAT of two Expected on the device, held against the host function's answer and returned"""
    host = binding.index_concat(indexed_of(a), indexed_of(b))
    got = plan.index_concat(_device_index(torch, a), _device_index(torch, b))
    assert got.nnz == host.nnz and np.array_equal(got.post_ptr.cpu().numpy().view(np.uint64), host.post_ptr), what
    assert np.array_equal(got.post_text.cpu().numpy().view(np.uint32)[:got.nnz], host.post_text), what
    assert np.array_equal(got.post_count.cpu().numpy().view(np.uint64)[:got.nnz], host.post_count), what
    plan.status()
    return got


def test_concat_on_the_device(torch_cuda, example, long_list):
    torch = torch_cuda
    m, plan, text, off, counts = example
    whole = nontrivial(counts, brute_force(counts, K))
    # the halves of the example; A over four keywords (the dictionary grew)
    a, b = brute_force(cut_rows(counts, 0, 7), K), brute_force(cut_rows(counts, 7, N), K, 7)
    assert a.nnz > 0 and b.nnz > 0
    check(_concat_both(torch, plan, a, b, "halves"), whole, "halves")
    a4 = brute_force(cut_rows(counts, 0, 7), 4)
    check(_concat_both(torch, plan, a4, b, "grown"), whole, "a dictionary that grew")
    # the 5,000-text batch cut at 2,500: both halves by the device's own transposition
    lm, ltext, loff, lcounts, ltexts = long_list
    lwhole = nontrivial(lcounts, brute_force(lcounts, K))
    lplan = lm.plan(0)
    halves = [lplan.index_matrix(_matrix(torch, tallied_of(cut_rows(lcounts, lo, hi))), text_base=lo) for lo, hi in ((0, 2500), (2500, len(ltexts)))]
    got = lplan.index_concat(halves[0], halves[1])
    check(got, lwhole, "5,000 texts cut at 2,500", total=False)
    host = binding.index_concat(*[binding.Indexed(h.post_ptr.cpu().numpy().view(np.uint64), h.post_text.cpu().numpy().view(np.uint32)[:h.nnz],
                                                  h.post_count.cpu().numpy().view(np.uint64)[:h.nnz], h.nnz) for h in halves])
    check(host, lwhole, "the host function on the same halves", total=False)
    lplan.status()
    # an overflow: the need, out_ptr complete, the guards stand; then count only
    L = acm.lib()
    A, B = _device_index(torch, a), _device_index(torch, b)
    n = whole.nnz

    def raw(plan, A, B, cap, room, fill=True, n_a=K, n_b=K):
        r = _Raw(torch, K, room)
        tb = L.acm_gpu_index_concat_tmp_bytes(plan.h, n_b)
        tmp = torch.empty(max(tb, 16), dtype=torch.uint8, device="cuda")
        rc = L.acm_gpu_index_concat_device(plan.h, A.post_ptr.data_ptr(), A.post_text.data_ptr(), A.post_count.data_ptr(), n_a, B.post_ptr.data_ptr(),
                                           B.post_text.data_ptr(), B.post_count.data_ptr(), n_b, r.p("post_ptr"), r.p("post_text") if fill else None,
                                           r.p("post_count") if fill else None, cap, r.res.data_ptr(), tmp.data_ptr(), tb, None)
        torch.cuda.synchronize()
        return rc, int(r.res[0].item()), r
    rc, found, r = raw(plan, A, B, n - 1, n - 1)
    assert rc == 0 and found == n and np.array_equal(r.host("post_ptr")[0].view(np.uint64), whole.post_ptr)
    r.guards_stand()
    rc, found, r = raw(plan, A, B, n, n)
    assert rc == 0 and found == n and np.array_equal(r.host("post_text")[0].view(np.uint32), whole.post_text)
    assert np.array_equal(r.host("post_count")[0].view(np.uint64), whole.post_count)
    r.guards_stand()
    rc, found, r = raw(plan, A, B, 0, n, fill=False)
    assert rc == 0 and found == n and np.array_equal(r.host("post_ptr")[0].view(np.uint64), whole.post_ptr)
    r.untouched("post_text", "post_count")
    plan.status()
    assert raw(plan, A, B, n, n, n_a=K, n_b=K - 1)[0] == binding.ACM_GPU_E_ARG
    # the violations: the flag is raised, *d_out_nnz = 0, nothing else is written
    low = _device_index(torch, brute_force(cut_rows(counts, 7, N), K, 0))               # B's `hers` begins with text 0, A's ends with 2
    down = binding.Indexed(_dev(torch, np.array([0, 3, 2, 5, 7, 7], np.uint64)), A.post_text, A.post_count, 7)
    for what, (x, y) in (("boundary", (A, low)), ("the same twice", (A, A)), ("a pointer array that decreases", (down, B)), ("B's decreases", (A, down))):
        fresh = m.plan(0)
        rc, found, r = raw(fresh, x, y, n, n)
        assert rc == 0 and found == 0, what
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        r.untouched("post_ptr", "post_text", "post_count")
