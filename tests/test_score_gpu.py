"""Weighted keyword scores per text on the GPU (acm_gpu_score_*, acm_score; csrc/dev_score.h).  The expected
kept matrix, BEST and TOP are always the brute-force evaluation, with Python integers modulo 2^64, of the
ORACLE's count matrix (tests/score_cases.py over tests/tally_batch_cases.expected), never of the library's own
counts; every workload case first shows from the oracle alone that it cannot pass trivially."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import score_class, weight
from tests.batch_cases import offsets_of, random_cuts
from tests.cases import build_pair
from tests.grep_cases import GREP_TEXTS
from tests.rules_cases import RULE_KEYWORDS
from tests.score_cases import EMPTY_COLUMN, EVERYWHERE, MODEL, check, check_top, expected_scored, nontrivial, wrapping_case
from tests.tally_batch_cases import expected
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind

pytestmark = pytest.mark.gpu

GUARD = 0x5A
GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
K = len(RULE_KEYWORDS)


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


def _texts(text, off):
    o = [int(x) for x in off]
    return [text[o[t]:o[t + 1]] for t in range(len(o) - 1)]


@pytest.fixture(scope="module")
def boundary():
    """(machine, plan, text, offsets, the oracle's count matrix, the model, expected) of the boundary set on a dense plan, made once"""
    m, o = build_pair(RULE_KEYWORDS, 1)
    text = np.frombuffer(b"".join(GREP_TEXTS), np.uint8)
    off = offsets_of(GREP_TEXTS)
    counts = expected(o, text, off)
    sm = binding.ScoreModel(MODEL)
    want = nontrivial(GREP_TEXTS, counts, sm, empty_column=EMPTY_COLUMN, everywhere=EVERYWHERE, ks=(1, 2), short_k=3)
    plan = m.plan(0)
    assert plan.info.kernel == 1, plan.describe()
    return m, plan, text, off, counts, sm, want


@pytest.mark.parametrize("items", [None, 1, 4])
def test_boundary_set_four_entry_points_fast_and_wide(torch_cuda, monkeypatch, boundary, items):
    """the boundary model in windows of 16 symbols; with a room of 1 or 4 items the texts that hold a keyword with more
    postings go through the wide form, which gives the oracle's matrix as the fast form does"""
    torch = torch_cuda
    m, plan, text, off, counts, sm, want = boundary
    if items:
        monkeypatch.setenv("ACM_GPU_SCORE_ITEMS", str(items))
    records = int(counts[2].sum())
    dev, d_off = _dev(torch, text), _dev(torch, off)
    S = plan.score_create(sm)
    info = S.info()
    assert (info["classes"], info["terms"], info["postings"], info["always_classes"]) == (8, 14, 14, 3) and info["fast_texts"] == info["wide_texts"] == 0
    calls = 0
    for k in (1, 2, 3):
        g = plan.score(dev, d_off, S, k=k, window=16, capacity=64, pair_capacity=records)
        calls += 2                                                         # (a count-only call first, then the call with room)
        assert 0 < g.need <= 64 and g.total == records
        check(g, want, ("Plan.score", items, k), k=k)
        plan.status()
    after = S.info()
    assert after["fast_texts"] + after["wide_texts"] == calls * (off.size - 1)
    if items:
        assert after["wide_texts"] > 0, after
    else:
        assert after["wide_texts"] == 0, after
    tallied = plan.tally_batch(dev, d_off, window=16, capacity=64, pair_capacity=records)
    g = plan.score_matrix(tallied, S)
    check(g, want, ("Plan.score_matrix", items))
    assert g.class_hits is None
    for k in (1, 2, 3):
        check_top(plan.score_top(g, sm.n_classes, k), want, k, ("Plan.score_top", items, k))
    plan.status()
    check(plan.score_matrix(tallied, sm), want, ("Plan.score_matrix, a model of its own", items))
    for k in (0, 2):
        h = plan.score_host(text, off, sm, k=k)
        check(h, want, ("Plan.score_host", items, k), k=k if k else None)
        assert h.total == records
    plan.status()
    got = m.score(GREP_TEXTS, sm, k=3)
    check(got, want, ("Machine.score", items), k=3)
    assert m.scan_path == PATH_GPU and got.total == records
    dense = g.to_sparse_csr(sm.n_classes).to_dense().cpu().numpy()
    assert all(dense[t][c] == (want.S[t][c] if want.keeps[t][c] else 0) for t in range(want.n_texts) for c in range(sm.n_classes))
    S.close()


@pytest.mark.parametrize("touched_always", [False, True])
@pytest.mark.parametrize("items", [None, 64, 4096])
def test_a_row_wider_than_a_wave(torch_cuda, monkeypatch, items, touched_always):
    """100 one-term classes on one keyword between 30 always-classes: rows of 130, 30 and 30 kept classes -- more
    outputs than a wave has lanes, the merge of the touched classes with the always-list, and with a room of 64
    items the wide form (4,096: the largest room, 64 KiB of LDS).  touched_always: 3 always-classes more ON the
    keyword, which its text touches and switches off (rows of 130, 33, 33)"""
    torch = torch_cuda
    if items:
        monkeypatch.setenv("ACM_GPU_SCORE_ITEMS", str(items))
    m, o = build_pair([b"ab", b"qq"], 1)
    classes, n_always = [], 0
    for i in range(130):
        if i % 4 == 1 and n_always < 30:
            classes.append(score_class([weight(1, 1)], bias=i, threshold=i))
            n_always += 1
        else:
            classes.append(score_class([weight(0, i + 1)]))
    if touched_always:
        for at in (0, 64, 133):
            classes.insert(at, score_class([weight(0, -5)], bias=1, threshold=1))
    sm = binding.ScoreModel(classes)
    texts = [b"xabx", b"xyz", b""]
    text, off = np.frombuffer(b"".join(texts), np.uint8), offsets_of(texts)
    counts = expected(o, text, off)
    want = expected_scored(counts, sm)
    extra = 3 if touched_always else 0
    assert np.diff(want.kept_ptr.astype(np.int64)).tolist() == [130, 30 + extra, 30 + extra]
    plan = m.plan(0)
    S = plan.score_create(sm)
    g = plan.score(_dev(torch, text), _dev(torch, off), S, k=2, window=16, capacity=64)
    check(g, want, ("wide row", items, touched_always), k=2)
    info = S.info()
    assert info["always_classes"] == 30 + extra and info["postings"] == 130 + extra
    wide = items == 64
    assert info["wide_texts"] == (2 if wide else 0) and info["fast_texts"] == (4 if wide else 6), info
    check(plan.score_host(text, off, sm, k=2), want, ("wide row, host", items, touched_always), k=2)
    plan.status()


@pytest.mark.parametrize("n_classes", [1, 100])
def test_a_column_longer_than_a_tile_with_ties(torch_cuda, monkeypatch, n_classes):
    """700 texts `s` and 5 texts `ss` under (s, weight, -): columns of 705, three tiles of the select pass; the top 5
    are the `ss` texts, behind them the lowest text ids in order.  With 100 classes and 7 blocks the grid strides."""
    torch = torch_cuda
    if n_classes > 1:
        monkeypatch.setenv("ACM_GPU_SCORE_TOP_BLOCKS", "7")
    m, o = build_pair([b"s", b"qq"], 1)
    texts = [b"s"] * 705
    twice = (100, 300, 301, 650, 704)
    for t in twice:
        texts[t] = b"ss"
    text, off = np.frombuffer(b"".join(texts), np.uint8), offsets_of(texts)
    counts = expected(o, text, off)
    sm = binding.ScoreModel([score_class([weight(0, c + 1)]) for c in range(n_classes)])
    want = expected_scored(counts, sm)
    assert want.class_hits.tolist() == [705] * n_classes
    top_n, top_text, top_score = want.top(64)
    singles = [t for t in range(705) if t not in twice]
    assert top_text[0].tolist() == list(twice) + singles[:59] and top_score[0][:6].tolist() == [2, 2, 2, 2, 2, 1]
    plan = m.plan(0)
    S = plan.score_create(sm)
    dev, d_off = _dev(torch, text), _dev(torch, off)
    for k in (1, 64, 256):
        g = plan.score(dev, d_off, S, k=k, window=256, capacity=1024, kept_capacity=705 * n_classes)
        check(g, want, ("long column", n_classes, k), k=k)
    plan.status()
    tallied = plan.tally_batch(dev, d_off, window=256, capacity=1024)
    check_top(plan.score_top(plan.score_matrix(tallied, S), n_classes, 256), want, 256, ("long column, score_top", n_classes))
    plan.status()
    S.close()


def _matrix(torch, t):
    col, val = np.asarray(t.col, np.uint32), np.asarray(t.val, np.uint64)
    return binding.TalliedBatch(_dev(torch, np.asarray(t.row_ptr, np.uint64)), _dev(torch, col) if col.size else torch.zeros(1, dtype=torch.int32, device="cuda"),
                                _dev(torch, val) if val.size else torch.zeros(1, dtype=torch.int64, device="cuda"), col.size, 0)


def test_a_wrapping_matrix_of_the_callers_own(torch_cuda):
    """counts of 2^40 and 2^63 under weights of +-(2^31 - 1): sums and products wrap modulo 2^64 on the device as in Python"""
    torch = torch_cuda
    tallied, sm, want = wrapping_case()
    m, o = build_pair([b"aa", b"bb", b"cc"], 1)
    plan = m.plan(0)
    g = plan.score_matrix(_matrix(torch, tallied), sm)
    check(g, want, "wrapping")
    for k in (1, 3):
        check_top(plan.score_top(g, sm.n_classes, k), want, k, ("wrapping", k))
    plan.status()
    # a col that is the model's n_keywords (a keyword the plan took later) is skipped, not flagged; no text at all
    two = binding.ScoreModel([score_class([weight(0, 2)]), score_class([weight(2, 3)], bias=1)])
    g = plan.score_matrix(_matrix(torch, binding.TalliedBatch(np.array([0, 2, 3, 3]), np.array([0, 3, 3]), np.array([1, 7, 9]), 3, 0)), two)
    assert g.kept_ptr.cpu().tolist() == [0, 2, 3, 4] and g.kept_class.cpu().tolist() == [0, 1, 1, 1] and g.kept_score.cpu().tolist() == [2, 1, 1, 1]
    assert g.best.cpu().tolist() == [0, 1, 1]
    g = plan.score_matrix(_matrix(torch, binding.TalliedBatch(np.array([0]), np.zeros(0), np.zeros(0), 0, 0)), two)
    assert g.n_kept == 0 and g.kept_ptr.cpu().tolist() == [0]
    plan.status()


class _Raw:
    """every output of acm_gpu_score_device / acm_gpu_score_matrix_device / acm_gpu_score_top_device in an array of guard
    values with 8 guard entries on either side of what the call may write"""

    def __init__(self, torch, n_texts, room, n_classes, k):
        self.torch, self.n_texts, self.room, self.n_classes, self.k = torch, n_texts, room, n_classes, k

        def guard(n, dtype):
            return torch.full((n + 16,), GUARD32 if dtype == torch.int32 else GUARD64, dtype=dtype, device="cuda")
        self.kept_ptr, self.kept_class, self.kept_score = guard(n_texts + 1, torch.int64), guard(room, torch.int32), guard(room, torch.int64)
        self.best, self.hits, self.top_n = guard(n_texts, torch.int32), guard(n_classes, torch.int64), guard(n_classes, torch.int32)
        self.top_text, self.top_score = guard(n_classes * k, torch.int32), guard(n_classes * k, torch.int64)
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
        for name in ("kept_ptr", "kept_class", "kept_score", "best", "hits", "top_n", "top_text", "top_score"):
            assert self.host(name)[1], name


def _raw_score(torch, plan, S, dev, d_off, n_texts, window, capacity, pair_capacity, kept_capacity, room, k):
    """acm_gpu_score_device into guarded arrays, the kept arrays with `room` entries; (rc, res = [n_kept, total, need, need_pairs], the _Raw)"""
    L = acm.lib()
    n = dev.numel()
    r = _Raw(torch, n_texts, room, S.n_classes, k)
    tb = L.acm_gpu_score_tmp_bytes(plan.h, S.h, window, capacity, pair_capacity, n, n_texts, kept_capacity, k)
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_score_device(plan.h, S.h, dev.data_ptr(), n, d_off.data_ptr(), n_texts, window, capacity, pair_capacity, r.p("kept_ptr"),
                                r.p("kept_class"), r.p("kept_score"), kept_capacity, r.res.data_ptr(), r.p("best"), k, r.p("hits"), r.p("top_n"),
                                r.p("top_text"), r.p("top_score"), r.res.data_ptr() + 8, r.res.data_ptr() + 16, r.res.data_ptr() + 24, tmp.data_ptr(), tb,
                                None)
    torch.cuda.synchronize()
    return rc, r.res.cpu().tolist(), r


def test_kept_overflow_on_the_device_and_guards(torch_cuda, boundary):
    torch = torch_cuda
    m, plan, text, off, counts, sm, want = boundary
    dev, d_off = _dev(torch, text), _dev(torch, off)
    n_texts, n, records = off.size - 1, want.n_kept, int(counts[2].sum())
    S = plan.score_create(sm)
    # one entry too little room: the need, kept_ptr complete, no byte outside the rooms, the top outputs zero
    rc, res, r = _raw_score(torch, plan, S, dev, d_off, n_texts, 16, 64, records, n - 1, n - 1, 3)
    assert rc == 0 and res[0] == n and res[1] == records and 0 < res[2] <= 64
    r.guards_stand()
    assert np.array_equal(r.host("kept_ptr")[0].view(np.uint64), want.kept_ptr)
    assert not r.host("hits")[0].any() and not r.host("top_n")[0].any()
    # exactly the room: the result, the guards around it stay
    rc, res, r = _raw_score(torch, plan, S, dev, d_off, n_texts, 16, 64, records, n, n, 3)
    assert rc == 0 and res[0] == n
    r.guards_stand()
    top_n, top_text, top_score = want.top(3)
    assert np.array_equal(r.host("kept_ptr")[0].view(np.uint64), want.kept_ptr) and np.array_equal(r.host("kept_class")[0].view(np.uint32), want.kept_class)
    assert np.array_equal(r.host("kept_score")[0], want.kept_score) and np.array_equal(r.host("best")[0].view(np.uint32), want.best)
    assert np.array_equal(r.host("hits")[0].view(np.uint64), want.class_hits) and np.array_equal(r.host("top_n")[0].view(np.uint32), top_n)
    assert np.array_equal(r.host("top_text")[0].view(np.uint32).reshape(-1, 3), top_text) and np.array_equal(r.host("top_score")[0].reshape(-1, 3), top_score)
    plan.status()
    # more partial pairs than room: what tally_batch reports, n_kept = 0, nothing else written
    rc, res, r = _raw_score(torch, plan, S, dev, d_off, n_texts, 16, 64, 1, n, n, 3)
    assert rc == 0 and res[0] == 0 and res[3] == records
    r.untouched("kept_ptr", "kept_class", "kept_score", "best", "hits", "top_n", "top_text", "top_score")
    plan.status()
    # Plan.score with a room that is too small says so in n_kept; count only
    g = plan.score(dev, d_off, S, k=2, window=16, capacity=64, pair_capacity=records, kept_capacity=n - 1)
    assert g.n_kept == n > g.kept_capacity and np.array_equal(g.kept_ptr.cpu().numpy().view(np.uint64), want.kept_ptr)
    assert not g.class_hits.cpu().numpy().any() and not g.top_n.cpu().numpy().any()
    g = plan.score(dev, d_off, S, k=2, window=16, capacity=64, pair_capacity=records, kept_capacity=0)
    assert g.n_kept == n and g.kept_class is None and g.class_hits is None
    # the host call: an overflow that leaves the kept arrays alone
    import ctypes as C
    fp, small, score, cnt, total = np.zeros(n_texts + 1, np.uint64), np.full(n - 1, GUARD32, np.uint32), np.full(n - 1, 77, np.int64), C.c_uint64(0), C.c_uint64(0)
    rc = acm.lib().acm_gpu_score_host(plan.h, text.ctypes.data, off.ctypes.data, n_texts, *sm.args(), fp.ctypes.data, small.ctypes.data, score.ctypes.data,
                                      n - 1, C.byref(cnt), None, 0, None, None, None, None, C.byref(total))
    assert rc == binding.ACM_GPU_E_OVERFLOW and cnt.value == n and total.value == records and np.array_equal(fp, want.kept_ptr)
    assert np.all(small == GUARD32) and np.all(score == 77)
    # arguments
    L = acm.lib()
    tmp = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, dtype=torch.int64, device="cuda")
    p = out.data_ptr()
    for kept_ptr, cls, score_p, cap, n_arg, nt, k in ((p, None, p + 512, 4, p + 1024, n_texts, 0), (p, p + 256, None, 4, p + 1024, n_texts, 0),
                                                      (None, p + 256, p + 512, 4, p + 1024, n_texts, 0), (p, p + 256, p + 512, 4, None, n_texts, 0),
                                                      (p, p + 256, p + 512, 4, p + 1024, 1 << 31, 0), (p, p + 256, p + 512, 4, p + 1024, n_texts, 257)):
        assert L.acm_gpu_score_device(plan.h, S.h, dev.data_ptr(), dev.numel(), d_off.data_ptr(), nt, 16, 64, 64, kept_ptr, cls, score_p, cap, n_arg, None,
                                      k, None, None, None, None, p + 1032, p + 1040, p + 1048, tmp.data_ptr(), tmp.numel(), None) == binding.ACM_GPU_E_ARG
    assert L.acm_gpu_score_matrix_tmp_bytes(plan.h, S.h, 1 << 31) == 0 and L.acm_gpu_score_tmp_bytes(plan.h, S.h, 16, 0, 8, text.size, n_texts, 8, 0) == 0
    assert L.acm_gpu_score_top_tmp_bytes(plan.h, 1 << 31, 8) == 0
    assert L.acm_gpu_score_top_device(plan.h, p, p + 256, p + 512, 4, n_texts, 8, 257, p + 1024, p + 1100, p + 1200, p + 1300, tmp.data_ptr(), tmp.numel(),
                                      None) == binding.ACM_GPU_E_ARG
    S.close()


def test_a_row_ptr_that_decreases_writes_nothing(torch_cuda):
    torch = torch_cuda
    m, o = build_pair([b"he", b"she"], 1)
    sm = binding.ScoreModel([score_class([weight(1, 1)]), score_class([weight(0, 1)], bias=1)])
    L = acm.lib()
    for what, bad in (("decreasing", [0, 2, 1, 3]), ("first", [1, 1, 2, 3])):
        fresh = m.plan(0)
        F = fresh.score_create(sm)
        mat = _matrix(torch, binding.TalliedBatch(np.array(bad), np.array([0, 1, 1]), np.array([1, 1, 1]), 3, 0))
        r = _Raw(torch, 3, 16, 2, 2)
        tb = L.acm_gpu_score_matrix_tmp_bytes(fresh.h, F.h, 3)
        tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
        rc = L.acm_gpu_score_matrix_device(fresh.h, F.h, mat.row_ptr.data_ptr(), mat.col.data_ptr(), mat.val.data_ptr(), 3, r.p("kept_ptr"),
                                           r.p("kept_class"), r.p("kept_score"), 16, r.res.data_ptr(), r.p("best"), tmp.data_ptr(), tb, None)
        assert rc == 0, what
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        assert int(r.res[0].item()) == 0, what
        r.untouched("kept_ptr", "kept_class", "kept_score", "best")
        # TOP of a kept_ptr that breaks the contract: the flag, nothing written; a class that is none: the flag, not counted
        fresh = m.plan(0)
        r = _Raw(torch, 3, 16, 2, 2)
        tb = L.acm_gpu_score_top_tmp_bytes(fresh.h, 16, 2)
        tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
        assert L.acm_gpu_score_top_device(fresh.h, mat.row_ptr.data_ptr(), r.p("kept_class"), r.p("kept_score"), 16, 3, 2, 2, r.p("hits"), r.p("top_n"),
                                          r.p("top_text"), r.p("top_score"), tmp.data_ptr(), tb, None) == 0
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        r.untouched("hits", "top_n", "top_text", "top_score")
        F.close()
    fresh = m.plan(0)
    kept = binding.Scored(_dev(torch, np.array([0, 2, 3], np.uint64)), _dev(torch, np.array([0, 2, 1], np.uint32)), _dev(torch, np.array([5, 6, 7], np.int64)), 3)
    top = fresh.score_top(kept, 2, 2)
    with pytest.raises(binding.ACMError) as e:
        fresh.status()
    assert e.value.code == -7
    assert top.class_hits.cpu().tolist() == [1, 1] and top.top_text.cpu().numpy().view(np.uint32).tolist() == [[0, 0xFFFFFFFF], [1, 0xFFFFFFFF]]


def _random_model(rng, keywords, n_classes):
    classes = []
    for c in range(n_classes):
        terms = [weight(int(keywords[int(rng.integers(0, len(keywords)))]), int(rng.integers(-9, 10)), [None, 1, 2, 5][int(rng.integers(0, 4))])
                 for _ in range(int(rng.integers(0, 6)))]
        classes.append(score_class(terms, bias=int(rng.integers(-3, 4)), threshold=int(rng.integers(-2, 6))))
    return classes


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram, CSR, start-parallel, sparse walk, 8-byte symbols, comparator classes, a plan with a pending delta --
    through Plan.score (four windows or more, one text over three whole windows) and Machine.score; a random model of 24
    classes over that kind's 8 most frequent keywords (by the oracle) and 2 that are rare"""
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
    n_keywords = o.nb_keywords
    order = np.argsort(-np.bincount(counts[1].astype(np.int64), weights=counts[2].astype(np.float64), minlength=n_keywords), kind="stable")
    sm = binding.ScoreModel(_random_model(np.random.default_rng(3), order[:8].tolist() + order[-2:].tolist(), 24))
    texts = _texts(text, off)
    want = nontrivial(texts, counts, sm)
    records = int(counts[2].sum())
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([np.zeros(1, text.dtype), text]))[1:]
        assert dev.data_ptr() % 16 == 1
    else:
        dev = _dev(torch_cuda, text)
    g = plan.score(dev, _dev(torch_cuda, off), sm, k=5, window=window, capacity=capacity, pair_capacity=records, kept_capacity=want.n_kept)
    print("kept %d, total %d, largest window %d, partial pairs %d" % (g.n_kept, g.total, g.need, g.need_pairs))
    assert 0 < g.need <= capacity and g.total == records
    check(g, want, "%s Plan.score" % name, k=5)
    plan.status()
    got = m.score(texts, sm, k=5)
    check(got, want, "%s Machine.score" % name, k=5)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU) and got.total == records
    plan.status()


def test_a_model_survives_a_plan_update(torch_cuda):
    """the model is created, then the machine gets a keyword that occurs in the texts and the plan takes it: the same
    Score gives the same result (the new keyword is in no term; its column is skipped)"""
    torch = torch_cuda
    m, o = build_pair(RULE_KEYWORDS, 1)
    text, off = np.frombuffer(b"".join(GREP_TEXTS), np.uint8), offsets_of(GREP_TEXTS)
    sm = binding.ScoreModel(MODEL)
    want = expected_scored(expected(o, text, off), sm)
    plan = m.plan(0)
    S = plan.score_create(sm)
    dev, d_off = _dev(torch, text), _dev(torch, off)
    check(plan.score(dev, d_off, S, k=2, window=16, capacity=64), want, "before the update", k=2)
    m.add_keyword(b"on")
    o.add_keyword(b"on")
    plan.update(m)
    assert plan.tally_keywords == K + 1
    after = expected(o, text, off)
    assert K in after[1].tolist()                                          # the new keyword occurs: "on top"
    g = plan.score(dev, d_off, S, k=2, window=16, capacity=64)
    assert g.total == int(after[2].sum())
    check(g, want, "after the update", k=2)
    plan.status()
    S.close()
