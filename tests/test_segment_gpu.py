"""The minimum-cost tiling on the GPU (acm_gpu_segment_*, acm_gpu_scan_segment_*, acm_segment;
csrc/dev_segment.h).  The expected answer is always the definition of SEGMENT in plain Python over the
ORACLE's records (tests/segment_cases.py), never the library's own scan.  Every case runs under three
settings of the two knobs: the defaults, ACM_GPU_SEGMENT_LONG=8 with ACM_GPU_SEGMENT_TILE=64 (both forms,
groups that straddle tile seams) and ACM_GPU_SEGMENT_LONG=1 (everything by the wave form)."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, TEXTS, offsets_of, oracle_batch
from tests.cases import build_pair
from tests.segment_cases import EXAMPLES, define, example, n_groups, random_cases
from tests.select_cases import assert_tiling, greedy, oracle_records
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, byte_oracle, kind
from tests.test_select_gpu import LETTERS, LONG, _seam_case

pytestmark = pytest.mark.gpu

E_ARG, E_INTERNAL = binding.ACM_GPU_E_ARG, -7
KNOBS = ["default", "long8_tile64", "long1"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(params=KNOBS)
def knobs(request, monkeypatch):
    monkeypatch.delenv("ACM_GPU_SEGMENT_LONG", raising=False)
    monkeypatch.delenv("ACM_GPU_SEGMENT_TILE", raising=False)
    if request.param == "long8_tile64":
        monkeypatch.setenv("ACM_GPU_SEGMENT_LONG", "8")
        monkeypatch.setenv("ACM_GPU_SEGMENT_TILE", "64")
    elif request.param == "long1":
        monkeypatch.setenv("ACM_GPU_SEGMENT_LONG", "1")
    return request.param


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


def _same(got, want):
    assert got.size == want.size and np.array_equal(got.astype(po.RECORD_DTYPE), want), (got.size, want.size, got[:8], want[:8])
    assert_tiling(got)


def _scan_segment(torch, plan, dev, cost, gap, capacity, **kw):
    """(records, (cost sum, length sum)) of Plan.scan_segment"""
    rec, cnt, sums, _ = plan.scan_segment(dev, _dev(torch, np.asarray(cost, np.uint32)), gap, capacity=capacity, **kw)
    n = int(cnt.item())
    assert n <= capacity, (n, capacity)
    return _rec_host(rec, n), (int(sums[0].item()), int(sums[1].item()))


def _sums_of(want, cost):
    return int(sum(int(cost[k]) for k in want["keyword_id"])), int(want["length"].astype(np.int64).sum())


@pytest.mark.parametrize("k", range(len(EXAMPLES)))
def test_worked_examples(torch_cuda, knobs, k):
    """`a` x 1001 and `a` x 1000 are one group of 2,001 and 2,997 records each: every chunk and ring seam of the
    wave form, and every step of the first a tie -- resolved from the left it puts the single `a` at the end"""
    rec, cost, gap, want, total, text, keywords = example(k)
    if k >= 2:
        assert n_groups(rec) == 1 and rec.size == (2001 if k == 2 else 2997)
    m, o = build_pair(keywords, 1)
    plan = m.plan(0)
    got, sums = _scan_segment(torch_cuda, plan, _dev(torch_cuda, text), cost, gap, rec.size)
    _same(got, want)
    assert sums[0] + gap * (len(text) - sums[1]) == total
    plan.status()


def test_many_small_groups(torch_cuda, knobs):
    """700 random letters, a separator no keyword holds every 3 to 9 symbols; every single letter and 30 random words"""
    rng = np.random.default_rng(700)
    text = bytearray(rng.integers(97, 123, size=700, dtype=np.uint8).tobytes())
    at = 0
    while True:
        at += int(rng.integers(3, 10))
        if at >= len(text):
            break
        text[at] = 32
        at += 1
    words = set()
    while len(words) < 30:
        s = int(rng.integers(0, len(text) - 5))
        w = bytes(text[s:s + int(rng.integers(2, 6))])
        if b" " not in w:
            words.add(w)                                           # (words the text holds: they compete with the letters)
    keywords = LETTERS + sorted(words)
    text = bytes(text)
    cost = np.concatenate([np.full(26, 3), 1 + 3 * (np.arange(30) % 7)]).astype(np.uint32)   # some words dearer than their letters
    m, o = build_pair(keywords, 1)
    rec = oracle_records(o, text)
    want, best = define(rec, cost, 5, 0, len(text))
    g = greedy(rec)
    print("records %d, groups %d, taken %d, SELECT takes %d" % (rec.size, n_groups(rec), want.size, g.size))
    assert n_groups(rec) >= 50 and not (g.size == want.size and np.array_equal(g, want))
    plan = m.plan(0)
    got, sums = _scan_segment(torch_cuda, plan, _dev(torch_cuda, text), cost, 5, rec.size)
    _same(got, want)
    assert sums == _sums_of(want, cost) and sums[0] + 5 * (len(text) - sums[1]) == best
    plan.status()


@pytest.mark.parametrize("depth,back", [(1, 27), (2, 65), (20, 513)])
def test_a_long_link_over_a_crowded_stretch(torch_cuda, knobs, depth, back):
    """test_select_gpu.py's seam case: single letters and the 40-symbol LONG, priced so that LONG is taken.  With the single
    letters alone its prev lies 27 records back (LONG's capitals are no keywords); with every piece of LONG of up to `depth`
    symbols as a keyword too, more than 64 back (depth 2) and more than 512 back (depth 20): the link leaves the wave form's
    chunk of 256 records and its ring of V"""
    keywords, text = _seam_case(b"")
    pieces = sorted({LONG[s:s + l] for l in range(2, depth + 1) for s in range(0, 40 - l + 1)})
    keywords = keywords[:-1] + pieces + [LONG]
    text = bytes(text)
    m, o = build_pair(keywords, 1)
    rec = oracle_records(o, text)
    cost = np.full(len(keywords), 2, np.uint32)
    cost[-1] = 3                                                   # LONG for 3 against two pieces or 40 letters for 2 each
    want, best = define(rec, cost, 9, 0, len(text))
    long_id = len(keywords) - 1
    taken = want[want["keyword_id"] == long_id]
    assert taken.size == 1
    i = int(np.flatnonzero((rec["keyword_id"] == long_id))[0])
    prev = int(np.searchsorted(rec["end_pos"], int(rec["end_pos"][i]) - 39)) - 1
    print("LONG is record %d, its prev record %d, %d back" % (i, prev, i - prev))
    assert prev >= 0 and i - prev >= back
    plan = m.plan(0)
    got, sums = _scan_segment(torch_cuda, plan, _dev(torch_cuda, text), cost, 9, rec.size)
    _same(got, want)
    assert sums[0] + 9 * (len(text) - sums[1]) == best
    plan.status()


def test_random_cases_through_segment_records(torch_cuda, knobs):
    """the 200 cases of the CPU test, the records uploaded, their count on the device"""
    torch = torch_cuda
    m, o = build_pair([b"abcdef", b"x"], 1)                        # lmax = 6: what the records' lengths may reach
    plan = m.plan(0)
    differ = 0
    for keywords, text, cost, gap in random_cases():
        rec = oracle_records(byte_oracle(keywords), text)
        want, _ = define(rec, cost, gap, 0, len(text))
        g = greedy(rec)
        differ += want.size > 0 and not (want.size == g.size and np.array_equal(want, g))
        room = rec.size + 3
        count = torch.tensor([rec.size], dtype=torch.int64, device="cuda")
        out, n, sums = plan.segment_records(_rec_dev(torch, rec, room), rec.size, 0, len(text), _dev(torch, cost), gap, count=count)
        _same(_rec_host(out, n), want)
        assert sums == _sums_of(want, cost)
    assert differ >= 100
    plan.status()


def test_the_result_does_not_depend_on_pos_lo(torch_cuda, knobs):
    torch = torch_cuda
    m, o = build_pair([b"abcdef", b"x"], 1)
    plan = m.plan(0)
    shift = 1 << 33
    for keywords, text, cost, gap in random_cases(seed=7, count=10):
        rec = oracle_records(byte_oracle(keywords), text)
        want, _ = define(rec, cost, gap)
        moved = rec.copy()
        moved["end_pos"] += shift
        for pos_lo, span in ((shift, len(text)), (shift - 1000, len(text) + 5000)):
            out, n, _ = plan.segment_records(_rec_dev(torch, moved), moved.size, pos_lo, span, _dev(torch, cost), gap)
            got = _rec_host(out, n)
            got["end_pos"] -= shift
            _same(got, want)
    plan.status()


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind(torch_cuda, knobs, monkeypatch, kat, novel_bytes, name):
    """scan_segment on the first 64 Ki symbols of the kind's text, costs 1 + (id % 5); default knobs also the host forms"""
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    text = text[:1 << 16]
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    if name == "csr":
        text = text[1:]
    rec = oracle_records(o, text)
    cost = (1 + np.arange(o.nb_keywords) % 5).astype(np.uint32)
    want, best = define(rec, cost, 8, 0, len(text))
    assert want.size > 0
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([text[:1], text]))[1:]                 # 1 byte past a 16-byte boundary
    else:
        dev = _dev(torch_cuda, text)
    got, sums = _scan_segment(torch_cuda, plan, dev, cost, 8, rec.size)
    _same(got, want)
    assert sums[0] + 8 * (len(text) - sums[1]) == best
    plan.status()
    if knobs == "default":
        got, sums = plan.scan_segment_host(text, cost, 8)
        _same(got, want)
        got, sums = m.segment(text, cost, 8)
        _same(got, want)
        assert sums == _sums_of(want, cost)
        assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)


def test_a_batch_is_the_concatenation_of_its_texts(torch_cuda, knobs):
    m, o = build_pair(KEYWORDS, 1)
    texts = TEXTS * 30
    off = offsets_of(texts)
    all_rec, _, first = oracle_batch(o, texts)
    cost = (1 + np.arange(len(KEYWORDS)) % 3).astype(np.uint32)
    per_text = []
    for t in range(len(texts)):
        r = all_rec[int(first[t]):int(first[t + 1])]
        per_text.append(define(r, cost, 2, int(off[t]), int(off[t + 1] - off[t]))[0])
    want = np.concatenate(per_text)
    assert 0 < want.size < all_rec.size
    plan = m.plan(0)
    flat = b"".join(texts)
    room = oracle_records(o, flat).size                            # the batch scan's rule: ALL matches of the buffer are found first
    assert room >= all_rec.size
    got, sums = _scan_segment(torch_cuda, plan, _dev(torch_cuda, flat), cost, 2, room, offsets=_dev(torch_cuda, off.astype(np.int64)))
    _same(got, want)
    assert sums == _sums_of(want, cost)
    got, _ = plan.scan_segment_host(np.frombuffer(flat, np.uint8), cost, 2, offsets=off)
    _same(got, want)
    plan.status()


def test_protocol_capacity_overflow_aliasing_and_no_sums(torch_cuda, knobs):
    torch = torch_cuda
    L = acm.lib()
    m, o = build_pair(KEYWORDS, 1)
    text = b"".join(TEXTS) * 50
    rec = oracle_records(o, text)
    cost = (1 + np.arange(len(KEYWORDS)) % 3).astype(np.uint32)
    want, _ = define(rec, cost, 2, 0, len(text))
    assert 0 < want.size < rec.size
    plan = m.plan(0)
    dev, d_cost = _dev(torch, text), _dev(torch, cost)
    # capacity - 1 names a capacity that suffices, and the repeat succeeds
    _, cnt, sums, _ = plan.scan_segment(dev, d_cost, 2, capacity=rec.size - 1)
    assert int(cnt.item()) == rec.size and sums.tolist() == [0, 0]
    got, _ = _scan_segment(torch, plan, dev, cost, 2, int(cnt.item()))
    _same(got, want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_segment_host(np.frombuffer(text, np.uint8), cost, 2, capacity=rec.size - 1)
    assert e.value.code == binding.ACM_GPU_E_OVERFLOW
    with pytest.raises(acm.ACMError):
        plan.scan_segment(dev, d_cost[:-1], 2, capacity=rec.size)        # the table does not cover the plan's keywords
    # *d_n > n_or_capacity: nothing is selected, the count stays, the sums are zero
    room = 64
    pattern = np.zeros(room, po.RECORD_DTYPE)
    pattern["end_pos"] = 0x0123456789ABCDEF
    count = torch.tensor([rec.size], dtype=torch.int64, device="cuda")
    sums = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    d_out = _rec_dev(torch, pattern)
    out, n, s = plan.segment_records(_rec_dev(torch, rec[:room]), room, 0, len(text), d_cost, 2, out=d_out, count=count, sums=sums)
    assert n == rec.size and s == (0, 0) and np.array_equal(_rec_host(d_out, room), pattern)
    # d_out == d_records, d_count == d_n
    d_rec = _rec_dev(torch, rec)
    count = torch.tensor([rec.size], dtype=torch.int64, device="cuda")
    out, n, s = plan.segment_records(d_rec, rec.size, 0, len(text), d_cost, 2, out=d_rec, count=count)
    assert out is d_rec and int(count.item()) == n
    _same(_rec_host(d_rec, n), want)
    assert s == _sums_of(want, cost)
    # d_sums == NULL
    d_rec = _rec_dev(torch, rec)
    d_out = _rec_dev(torch, pattern, rec.size)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_segment_tmp_bytes(plan.h, rec.size, len(text))
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call(plan_h=plan.h, records=d_rec.data_ptr(), n=rec.size, span=len(text), d_c=d_cost.data_ptr(), nk=cost.size, gap=2, out=d_out.data_ptr(),
             cnt=count.data_ptr(), scratch=tmp.data_ptr(), tmp_bytes=tb):
        return L.acm_gpu_segment_records_device(plan_h, records, n, None, 0, span, d_c, nk, gap, out, cnt, None, scratch, tmp_bytes, None)
    assert call(plan_h=None) == E_ARG and call(records=None) == E_ARG and call(out=None) == E_ARG and call(cnt=None) == E_ARG
    assert call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG and call(span=0) == E_ARG
    assert call(d_c=None) == E_ARG and call(gap=1 << 24) == E_ARG
    assert L.acm_gpu_segment_tmp_bytes(plan.h, 1 << 31, 64) == 0 and L.acm_gpu_scan_segment_tmp_bytes(plan.h, 1 << 31, 64, 0) == 0
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and np.array_equal(_rec_host(d_out, 8)["end_pos"], pattern["end_pos"][:8])     # nothing was touched
    assert call() == 0
    torch.cuda.synchronize()
    _same(_rec_host(d_out, int(count.item())), want)
    # n = 0, an empty text and a text without a match
    out, n, s = plan.segment_records(d_rec, 0, 0, len(text), d_cost, 2)
    assert (n, s) == (0, (0, 0))
    empty = _dev(torch, np.zeros(16, np.uint8))[:0]
    assert _scan_segment(torch, plan, empty, cost, 2, 16)[0].size == 0
    got, s = _scan_segment(torch, plan, _dev(torch, b"q" * 3000), cost, 2, 16)
    assert got.size == 0 and s == (0, 0)
    got, s = m.segment(b"qqqq", cost, 2)
    assert got.size == 0 and s == (0, 0)
    plan.status()


def test_contract_violations_are_rejected_by_the_validation_pass(torch_cuda, knobs):
    """a keyword_id beyond n_keywords, a device cost of 2^24: hand-made inputs the validation pass rejects before any
    address or sum is formed from them.  Status ACM_GPU_E_INTERNAL, count 0, the canaries around every output intact."""
    torch = torch_cuda
    L = acm.lib()
    m, o = build_pair(KEYWORDS, 1)
    text = b"".join(TEXTS) * 5
    rec = oracle_records(o, text)
    cost = np.ones(len(KEYWORDS), np.uint32)
    bad_kw = rec.copy()
    bad_kw["keyword_id"][rec.size // 2] = 0x7FFFFFF0
    bad_cost = cost.copy()
    bad_cost[int(rec["keyword_id"][0])] = 1 << 24
    CANARY = 0x5A5A5A5A5A5A5A5A
    for records, table in ((bad_kw, cost), (rec, bad_cost)):
        plan = m.plan(0)
        n = records.size
        out = torch.full((n + 16, 2), CANARY, dtype=torch.int64, device="cuda")       # 8 canary records on either side
        count = torch.full((3,), CANARY, dtype=torch.int64, device="cuda")
        sums = torch.full((4,), CANARY, dtype=torch.int64, device="cuda")
        d_rec, d_cost = _rec_dev(torch, records), _dev(torch, table)
        tb = L.acm_gpu_segment_tmp_bytes(plan.h, n, len(text))
        tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
        rc = L.acm_gpu_segment_records_device(plan.h, d_rec.data_ptr(), n, None, 0, len(text), d_cost.data_ptr(), table.size, 1,
                                              out[8:].data_ptr(), count[1:].data_ptr(), sums[1:].data_ptr(), tmp.data_ptr(), tb, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert count.tolist() == [CANARY, 0, CANARY]
        assert bool((out == CANARY).all()) and bool((sums == CANARY).all())           # nothing else was written
        assert np.array_equal(_rec_host(d_rec, n), records)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL
        plan.close()


def test_two_runs_give_the_same_bytes(torch_cuda, knobs):
    torch = torch_cuda
    rec, cost, gap, want, total, text, keywords = example(3)
    m, o = build_pair(keywords, 1)
    plan = m.plan(0)
    runs = []
    for _ in range(2):
        records = torch.zeros((rec.size, 2), dtype=torch.int64, device="cuda")
        r, cnt, sums, _ = plan.scan_segment(_dev(torch, text), _dev(torch, cost), gap, records=records)
        runs.append((r.cpu().numpy().tobytes(), int(cnt.item()), sums.tolist()))
    assert runs[0] == runs[1]
    plan.status()


def test_composition_with_the_token_pass(torch_cuda, knobs):
    """scan_segment, then Plan.tokens_records (mode "run") on the device: a unigram tokeniser"""
    torch = torch_cuda
    keywords = [b"he", b"she", b"his", b"hers", b"us", b"her"]
    text = b"ushers shershis hehers us " * 40
    m, o = build_pair(keywords, 1)
    rec = oracle_records(o, text)
    cost = np.array([3, 4, 4, 2, 3, 5], np.uint32)
    want, _ = define(rec, cost, 6, 0, len(text))
    g = greedy(rec)
    assert want.size > 0 and not (g.size == want.size and np.array_equal(g, want))
    plan = m.plan(0)
    dev = _dev(torch, text)
    records, cnt, _, _ = plan.scan_segment(dev, _dev(torch, cost), 6, capacity=rec.size)
    n = int(cnt.item())
    _same(_rec_host(records, n), want)
    got = plan.tokens_records(dev, records, n, gap_base=100, mode="run")
    ref = binding.tokens_records(np.frombuffer(text, np.uint8), want, gap_base=100, mode="run")
    k = int(ref.n_tokens)
    assert got.n_tokens == k and k > want.size
    for mine, theirs in ((got.ids, ref.ids), (got.start, ref.start), (got.length, ref.length)):
        assert np.array_equal(mine[:k].cpu().numpy().astype(np.int64), np.asarray(theirs).astype(np.int64))
    plan.status()
