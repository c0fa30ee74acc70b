"""Leftmost-longest selection on the GPU (acm_gpu_select_*, acm_gpu_scan_select_*, acm_select;
csrc/dev_select.h).  The expected answer is always the definition of SELECT in plain Python over the
ORACLE's records (tests/select_cases.py), never the library's own scan; every workload case first
shows from the oracle alone that something is selected and something is left out."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, TEXTS, offsets_of, oracle_batch
from tests.cases import build_pair
from tests.select_cases import assert_tiling, greedy, nontrivial, oracle_records, random_case
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind

pytestmark = pytest.mark.gpu

E_ARG, E_INTERNAL = binding.ACM_GPU_E_ARG, -7
FORM_TILED, FORM_WALK = 1, 2
LONG = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMN"          # 40 symbols (test_tally_gpu.py's)
LETTERS = [bytes([c]) for c in range(97, 123)]


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


def _same(got, want):
    assert got.size == want.size and np.array_equal(got.astype(po.RECORD_DTYPE), want), (got.size, want.size, got[:8], want[:8])
    assert_tiling(got)


def _scan_select(plan, dev, capacity, **kw):
    rec, cnt, _ = plan.scan_select(dev, capacity=capacity, **kw)
    n = int(cnt.item())
    assert n <= capacity, (n, capacity)
    return _rec_host(rec, n)


def _mode(monkeypatch, mode):
    """the three ways a selection can run here; returns the form select_form must report"""
    monkeypatch.delenv("ACM_GPU_SELECT", raising=False)
    monkeypatch.delenv("ACM_GPU_SELECT_TILE", raising=False)
    if mode == "tile64":
        monkeypatch.setenv("ACM_GPU_SELECT_TILE", "64")
    elif mode == "walk":
        monkeypatch.setenv("ACM_GPU_SELECT", "walk")
    else:
        assert mode == "default"
    return FORM_WALK if mode == "walk" else FORM_TILED


MODES = ["tile64", "default", "walk"]


@pytest.mark.parametrize("mode", MODES)
def test_parity_entry_offsets(torch_cuda, monkeypatch, mode):
    """{aa} on a x 1000: 500 records at the even starts; {aa, aaa}: 333 records of length 3 at the starts
    0, 3, ..., 996 -- a tile of 64 candidates is entered at offset 0, 2, 1, 0, ... in turn, so a tile
    map taken as constant fails here"""
    text = b"a" * 1000
    form = _mode(monkeypatch, mode)
    for keywords, n_sel, step in (([b"aa"], 500, 2), ([b"aa", b"aaa"], 333, 3)):
        m, o = build_pair(keywords, 1)
        rec = oracle_records(o, text)
        want = greedy(rec)
        nontrivial(rec, want)
        assert want.size == n_sel and np.all(want["length"] == step)
        assert np.array_equal(want["end_pos"].astype(np.int64) + 1 - step, np.arange(n_sel) * step)
        plan = m.plan(0)
        assert plan.select_form == form
        _same(_scan_select(plan, _dev(torch_cuda, text), rec.size), want)
        plan.status()


def _seam_case(extra):
    """every single letter a-z (and `extra` single letters), plus LONG; LONG begins 3 candidates in front
    of the seam between the first two tiles of 64 candidates and again in front of a later seam"""
    keywords = LETTERS + [bytes([c]) for c in extra] + [LONG]
    rng = np.random.default_rng(40)
    text = bytearray(rng.integers(97, 123, size=700, dtype=np.uint8).tobytes())
    text[61:61 + 40] = LONG
    return keywords, text


@pytest.mark.parametrize("extra", [b"", b"ABCDEFGHIJKLMN"], ids=["a-z", "a-zA-N"])
def test_long_jump_over_a_crowded_tile_seam(torch_cuda, monkeypatch, extra):
    keywords, text = _seam_case(extra)
    # a second LONG in front of a later seam: where the candidate (= distinct start) with index = -3 mod 64 lies
    m, o = build_pair(keywords, 1)
    starts = np.unique(oracle_records(o, bytes(text))["end_pos"].astype(np.int64) + 1 - oracle_records(o, bytes(text))["length"])
    at = int(starts[64 * 5 - 3])
    text[at:at + 40] = LONG
    text = bytes(text)
    rec = oracle_records(o, text)
    want = greedy(rec)
    nontrivial(rec, want)
    starts = np.unique(rec["end_pos"].astype(np.int64) + 1 - rec["length"])
    long_id = len(keywords) - 1
    jumps = want[want["keyword_id"] == long_id]
    assert jumps.size == 2                                                          # both are selected ...
    for j in jumps:
        s, e = int(j["end_pos"]) - 39, int(j["end_pos"]) + 1
        i, nxt = int(np.searchsorted(starts, s)), int(np.searchsorted(starts, e))
        print("LONG at candidate %d jumps to %d: enters the next tile at offset %d" % (i, nxt, nxt % 64))
        assert i % 64 == 61 and nxt // 64 == i // 64 + 1                            # ... 3 in front of a seam of 64, into the next tile
        assert nxt % 64 == (37 if extra else 23)                                    # deep inside it: near lmax - 1 = 39 with A-N as starts
    plan = m.plan(0)
    dev = _dev(torch_cuda, text)
    got = {}
    for tile, form in ((64, FORM_TILED), (32, FORM_WALK)):                          # lmax = 40 > 32: the general form
        monkeypatch.setenv("ACM_GPU_SELECT_TILE", str(tile))
        assert plan.select_form == form
        got[tile] = _scan_select(plan, dev, rec.size)
        _same(got[tile], want)
    monkeypatch.setenv("ACM_GPU_SELECT_TILE", "64")
    monkeypatch.setenv("ACM_GPU_SELECT", "walk")
    assert plan.select_form == FORM_WALK
    _same(_scan_select(plan, dev, rec.size), want)
    monkeypatch.delenv("ACM_GPU_SELECT")
    monkeypatch.delenv("ACM_GPU_SELECT_TILE")
    assert plan.select_form == FORM_TILED                                           # the default tile holds lmax = 40
    _same(_scan_select(plan, dev, rec.size), want)
    plan.status()


def _hand_made(rng, bases, per_cluster, lmax):
    """records in canonical order: clusters of overlapping records, distinct (end_pos, length) pairs"""
    seen = set()
    for b in bases:
        for _ in range(per_cluster):
            length = int(rng.integers(1, lmax + 1))
            seen.add((int(b + rng.integers(lmax, 60)), length))
    rows = sorted(seen, key=lambda r: (r[0], -r[1]))
    rec = np.zeros(len(rows), po.RECORD_DTYPE)
    rec["end_pos"] = [r[0] for r in rows]
    rec["length"] = [r[1] for r in rows]
    rec["keyword_id"] = rng.integers(0, 1 << 20, size=len(rows))
    return rec


@pytest.mark.parametrize("mode", MODES)
def test_select_records_on_hand_made_records(torch_cuda, monkeypatch, mode):
    form = _mode(monkeypatch, mode)
    m, o = build_pair([b"ab", b"abcdefgh", b"x"], 1)                                 # lmax = 8: what the records' lengths may reach
    plan = m.plan(0)
    assert plan.select_form == form
    rng = np.random.default_rng(13)
    pos_lo, span = 500, 4_000_000
    # gaps of thousands of positions between clusters; a crowd of 3,000 records in one of them
    bases = [pos_lo, 1500, 9000, 9100, 50_000, 1_000_000, 1_004_096, 3_999_900]
    rec = np.concatenate([_hand_made(rng, bases, 40, 8), _hand_made(rng, [2_000_000 + 37 * i for i in range(100)], 30, 8)])
    rec = rec[np.lexsort((-rec["length"].astype(np.int64), rec["end_pos"]))]                # (the two sets share no position)
    want = greedy(rec)
    nontrivial(rec, want)
    assert rec.size > 2000 and int(rec["end_pos"].max()) < pos_lo + span
    dev = _rec_dev(torch_cuda, rec)
    out, n = plan.select_records(dev, rec.size, pos_lo, span)
    _same(_rec_host(out, n), want)
    assert np.array_equal(_rec_host(dev, rec.size), rec)                             # the input is left as it was
    # d_out aliased to d_records
    out, n = plan.select_records(dev, rec.size, pos_lo, span, out=dev)
    assert out is dev
    _same(_rec_host(dev, n), want)
    # one record only, and none
    one = np.array([(pos_lo + 7, 8, 5)], po.RECORD_DTYPE)
    out, n = plan.select_records(_rec_dev(torch_cuda, one), 1, pos_lo, span)
    _same(_rec_host(out, n), one)
    out, n = plan.select_records(_rec_dev(torch_cuda, one), 0, pos_lo, span)
    assert n == 0
    plan.status()


def test_a_record_that_starts_below_pos_lo_is_dropped_and_reported(torch_cuda):
    m, o = build_pair([b"ab", b"abcdefgh", b"x"], 1)
    plan = m.plan(0)
    pos_lo, span = 1000, 5000
    good = _hand_made(np.random.default_rng(5), [pos_lo, 1100, 3000], 40, 8)
    good = good[good["end_pos"].astype(np.int64) + 1 - good["length"] >= pos_lo]
    want = greedy(good)
    nontrivial(good, want)
    bad = np.array([(pos_lo + 2, 8, 77)], po.RECORD_DTYPE)                           # starts 5 positions below pos_lo
    rec = np.concatenate([good, bad])
    rec = rec[np.lexsort((-rec["length"].astype(np.int64), rec["end_pos"]))]
    assert greedy(rec)[0]["keyword_id"] == 77                                        # (kept, it would be the first record selected)
    out, n = plan.select_records(_rec_dev(torch_cuda, rec), rec.size, pos_lo, span)
    _same(_rec_host(out, n), want)
    with pytest.raises(acm.ACMError) as e:
        plan.status()
    assert e.value.code == E_INTERNAL


def test_random_differential_at_tile_64(torch_cuda, monkeypatch):
    monkeypatch.setenv("ACM_GPU_SELECT_TILE", "64")
    rng = np.random.default_rng(67)                                                  # (a seed whose 40 cases all leave something out)
    for case in range(40):
        keywords, text = random_case(rng, 12, 9, 5000)
        m, o = build_pair(keywords, 1)
        rec = oracle_records(o, text)
        want = greedy(rec)
        nontrivial(rec, want)
        plan = m.plan(0)
        assert plan.select_form == FORM_TILED
        _same(_scan_select(plan, _dev(torch_cuda, text), rec.size), want)
        plan.status()
        plan.close()


def _overlap_across_the_delta(text):
    """the delta case's 450 keywords leave no two overlapping matches in the first 1 << 18 symbols of the
    synthetic text: a keyword of the plan's own tables (the first 300) is written into a copy of the text
    with a keyword of the delta (300 .. 448) beginning on its last symbol, so that one record of each
    overlap and the selection has to drop the delta's"""
    kd, ko = acm.synth.keywords(450)
    a, b = next((a, b) for a in range(300) for b in range(300, 449) if kd[ko[a + 1] - 1] == kd[ko[b]] and ko[b + 1] - ko[b] > 1)
    both = np.concatenate([kd[ko[a]:ko[a + 1]], kd[ko[b] + 1:ko[b + 1]]])
    text = text.copy()
    text[100_000:100_000 + both.size] = both
    return text


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind_three_entry_points(torch_cuda, monkeypatch, kat, novel_bytes, name):
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    text = text[:1 << 18]
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    assert plan.select_form == FORM_TILED
    if name == "csr":
        text = text[1:]
    if name == "delta":
        text = _overlap_across_the_delta(text)
    rec = oracle_records(o, text)
    want = greedy(rec)
    nontrivial(rec, want)
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([text[:1], text]))[1:]                 # 1 byte past a 16-byte boundary
        assert dev.data_ptr() % 16 == 1 and dev.is_contiguous()
    else:
        dev = _dev(torch_cuda, text)
    _same(_scan_select(plan, dev, rec.size), want)
    plan.status()
    _same(plan.scan_select_host(text), want)
    _same(plan.scan_select_host(text, capacity=rec.size), want)
    _same(m.select(text), want)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)


def test_overflow_reports_a_capacity_that_suffices(torch_cuda):
    m, o = build_pair(KEYWORDS, 1)
    text = b"".join(TEXTS) * 50
    rec = oracle_records(o, text)
    want = greedy(rec)
    nontrivial(rec, want)
    plan = m.plan(0)
    dev = _dev(torch_cuda, text)
    _, cnt, _ = plan.scan_select(dev, capacity=rec.size - 1)
    assert int(cnt.item()) == rec.size                                               # the all-match count, not the selection's
    _same(_scan_select(plan, dev, int(cnt.item())), want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_select_host(np.frombuffer(text, np.uint8), capacity=rec.size - 1)
    assert e.value.code == binding.ACM_GPU_E_OVERFLOW
    with pytest.raises(acm.ACMError):
        m.select(text, capacity=want.size)                                           # room for the selection alone is not enough
    _same(m.select(text, capacity=rec.size), want)
    # an empty text and a text without a match
    empty = _dev(torch_cuda, np.zeros(16, np.uint8))[:0]
    assert _scan_select(plan, empty, 16).size == 0
    assert _scan_select(plan, _dev(torch_cuda, b"q" * 3000), 16).size == 0
    assert plan.scan_select_host(np.zeros(0, np.uint8)).size == 0 and m.select(b"qqqq").size == 0
    plan.status()


def test_select_of_a_batch_is_the_concatenation_of_the_texts_selections(torch_cuda):
    m, o = build_pair(KEYWORDS, 1)
    texts = TEXTS * 30
    off = offsets_of(texts)
    all_rec, _, first = oracle_batch(o, texts)
    per_text = [greedy(all_rec[int(first[t]):int(first[t + 1])]) for t in range(len(texts))]
    want = np.concatenate(per_text)
    nontrivial(all_rec, want)
    plan = m.plan(0)
    rec, _, _ = plan.scan_batch(_dev(torch_cuda, b"".join(texts)), _dev(torch_cuda, off.astype(np.int64)))
    assert np.array_equal(rec, all_rec)
    out, n = plan.select_records(_rec_dev(torch_cuda, rec), rec.size, 0, int(off[-1]))
    _same(_rec_host(out, n), want)
    plan.status()


def test_select_device_arguments(torch_cuda):
    torch = torch_cuda
    m, o = build_pair([b"he", b"she"], 1)
    plan = m.plan(0)
    L = acm.lib()
    text = b"ushers" * 10
    dev = _dev(torch, text)
    rec = oracle_records(o, text)
    pattern = np.zeros(64, po.RECORD_DTYPE)
    pattern["end_pos"] = 0x0123456789ABCDEF
    d_rec = _rec_dev(torch, rec, 64)
    d_out = _rec_dev(torch, pattern)
    count = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_select_tmp_bytes(plan.h, 64, len(text))
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def select(plan_h=plan.h, records=d_rec.data_ptr(), n=rec.size, out=d_out.data_ptr(), cnt=count.data_ptr(), scratch=tmp.data_ptr(),
               tmp_bytes=tb, span=len(text)):
        return L.acm_gpu_select_records_device(plan_h, records, n, None, 0, span, out, cnt, scratch, tmp_bytes, None)
    tb_n = L.acm_gpu_select_tmp_bytes(plan.h, rec.size, len(text))
    assert 0 < tb_n <= tb
    assert select(plan_h=None) == E_ARG and select(records=None) == E_ARG and select(out=None) == E_ARG
    assert select(cnt=None) == E_ARG and select(scratch=None) == E_ARG
    assert select(tmp_bytes=tb_n - 1) == E_ARG and select(n=1 << 31) == E_ARG and select(span=0) == E_ARG
    assert L.acm_gpu_select_tmp_bytes(plan.h, 1 << 31, 64) == 0 and L.acm_gpu_scan_select_tmp_bytes(plan.h, 1 << 31, 64) == 0

    stb = L.acm_gpu_scan_select_tmp_bytes(plan.h, 64, len(text))
    stmp = torch.empty(stb, dtype=torch.uint8, device="cuda")

    def scan_select(plan_h=plan.h, txt=dev.data_ptr(), records=d_out.data_ptr(), capacity=64, cnt=count.data_ptr(), scratch=stmp.data_ptr(),
                    tmp_bytes=stb):
        return L.acm_gpu_scan_select_device(plan_h, txt, len(text), 0, records, capacity, cnt, scratch, tmp_bytes, None)
    assert scan_select(plan_h=None) == E_ARG and scan_select(txt=None) == E_ARG and scan_select(records=None) == E_ARG
    assert scan_select(cnt=None) == E_ARG and scan_select(scratch=None) == E_ARG
    assert scan_select(tmp_bytes=stb - 1) == E_ARG and scan_select(capacity=1 << 31) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(_rec_host(d_out, 64), pattern) and int(count.item()) == 0x5A5A      # nothing was touched
    want = greedy(rec)
    assert select() == 0
    torch.cuda.synchronize()
    _same(_rec_host(d_out, int(count.item())), want)
    assert scan_select() == 0
    torch.cuda.synchronize()
    _same(_rec_host(d_out, int(count.item())), want)
    plan.status()
