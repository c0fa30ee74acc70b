"""grep over a batch on the GPU (acm_gpu_grep_*, acm_grep; csrc/dev_grep.h).  The expected answer is
always derived from the ORACLE's scan of every text alone (tests/grep_cases.py: hits = np.diff (first),
the rest in numpy), never from the library's own scan; every workload case first shows from the oracle
alone that it cannot pass trivially (a text that is not empty without a hit, two distinct non-zero
hit counts, a match of the concatenation across a text boundary, both KEPT sets non-empty)."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import offsets_of, oracle_batch, oracle_batch_cut, random_cuts
from tests.cases import build_pair
from tests.grep_cases import check, expected, nontrivial, oracle_hits
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind

pytestmark = pytest.mark.gpu

E_ARG = binding.ACM_GPU_E_ARG
GUARD = 0xA5


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


def _off_at(torch, arr, k):
    """`arr` on the device, its first symbol k symbols past a 16-byte boundary"""
    a = np.ascontiguousarray(arr)
    d = _dev(torch, np.concatenate([np.zeros(k, a.dtype), a]))[k:]
    assert d.data_ptr() % 16 == (k * a.itemsize) % 16 and d.is_contiguous()
    return d


def _np(g, sb):
    """a Grepped of device tensors -> one of numpy arrays cut to size"""
    hits = g.hits.cpu().numpy().view(np.uint64).copy()
    kept = g.kept[:g.n_kept].cpu().numpy().view(np.uint32).copy()
    off = g.out_offsets[:g.n_kept + 1].cpu().numpy().view(np.uint64).copy()
    out = None
    if g.out is not None and g.out_symbols <= g.out_capacity:
        out = g.out.reshape(-1)[:g.out_symbols * sb // g.out.element_size()].cpu().numpy().copy()
    return binding.Grepped(hits, kept, g.n_kept, g.total, g.need, out, off, g.out_symbols, g.out_capacity)


def _texts(text, off):
    o = [int(x) for x in off]
    return [text[o[t]:o[t + 1]] for t in range(len(o) - 1)]


_cases = {}


def _workload(name, monkeypatch, kat, novel_bytes):
    """(machine, oracle, text, plan, offsets, oracle hits) of a plan kind; the dense one is made once
    and shared (its answer also feeds the composition test)"""
    if name == "dense" and name in _cases:
        return _cases[name]
    m, o, text, make_plan, plan_ok, form = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    if name == "csr":
        text = text[1:]
    if name == "classes":
        # the novel cut at its newlines, some cuts doubled (empty texts), and five cuts inside a match
        # (no match holds a newline: without them nothing would cross a boundary)
        nl = np.flatnonzero(text == 10) + 1
        whole = o.scan(text)
        long_ones = whole[whole["length"] >= 3]
        inside = long_ones["end_pos"][:: max(long_ones.size // 5, 1)][:5].astype(np.int64)
        off = np.sort(np.concatenate([[0, 0], nl, nl[::50], inside, [text.size, text.size]])).astype(np.uint64)
    else:
        off = random_cuts(text.size, 700)
    assert np.any(off[1:] == off[:-1]) and off[0] == 0 and off[-1] == text.size
    hits = oracle_hits(o, text, off)
    nontrivial(o, text, off, hits)
    case = (m, o, text, plan, off, hits)
    if name == "dense":
        _cases[name] = case
    return case


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind_three_entry_points(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram, CSR (a dense plan on a pointer off the 16-byte grid, also at every window),
    start-parallel, sparse walk, 8-byte symbols, comparator classes, a plan with a pending delta --
    through Plan.grep (four windows or more), Plan.grep_host and Machine.grep, with both flags"""
    m, o, text, plan, off, hits = _workload(name, monkeypatch, kat, novel_bytes)
    sb = text.itemsize
    dev = _off_at(torch_cuda, text, 1 if name == "csr" else 0)
    d_off = _dev(torch_cuda, off)
    window = capacity = 1 << 16
    assert text.size > 3 * window
    for invert in (False, True):
        want = expected(text, off, hits, invert)
        g = plan.grep(dev, d_off, invert=invert, window=window, capacity=capacity)
        print("invert %d: kept %d of %d, total %d, largest window %d, out symbols %d" % (invert, g.n_kept, hits.size, g.total, g.need, g.out_symbols))
        assert 0 < g.need <= capacity
        check(_np(g, sb), hits, want, sb, "%s Plan.grep invert=%d" % (name, invert))
        plan.status()
        check(plan.grep_host(text, off, invert=invert), hits, want, sb, "%s Plan.grep_host invert=%d" % (name, invert))
        check(m.grep(_texts(text, off), invert=invert), hits, want, sb, "%s Machine.grep invert=%d" % (name, invert))
        assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    plan.status()


def test_composition_gathered_buffer_feeds_the_batch_scan(torch_cuda, monkeypatch, kat, novel_bytes):
    m, o, text, plan, off, hits = _workload("dense", monkeypatch, kat, novel_bytes)
    g = plan.grep(_dev(torch_cuda, text), _dev(torch_cuda, off), window=1 << 16, capacity=1 << 16)
    kept, out_off, out = expected(text, off, hits, False)
    assert g.n_kept == kept.size and g.out_symbols == out.size
    texts = _texts(text, off)
    want = oracle_batch(o, [texts[t] for t in kept])
    got = plan.scan_batch(g.out[:g.out_symbols], g.out_offsets[:g.n_kept + 1])
    for a, b, what in zip(got, want, ("records", "text_id", "first")):
        assert a.shape == b.shape and np.array_equal(a, b), what
    assert np.array_equal(np.diff(got[2].astype(np.int64)), hits[kept].astype(np.int64))
    plan.status()


LONG = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMN"          # 40 symbols


def test_window_cuts_and_text_cuts_together(torch_cuda):
    keywords = [b"he", b"she", b"hers", b"s", LONG]
    # tests/test_tally_gpu.py::test_window_cuts_lose_and_double_nothing's text: the long keyword from 10, from 100 and at the end
    text = b"ushers he " + LONG + b" she sells hers; his ushers she hers ssh" + b"x" * 10 + LONG + b" hers she " * 9 + b"she" + LONG
    n = len(text)
    assert text[10:50] == LONG and text[100:140] == LONG and text[n - 40:] == LONG and n == 273
    m, o = build_pair(keywords, 1)
    # [5, 60) holds the first long keyword and spans the window boundaries 16, 32 and 48; the cut at 112 goes
    # through the second; 96 and 192 are boundaries of the windows of 16 and of 48, 112 of those of 16; [96, 112)
    # has no match; empty texts at the front, in the middle and at the end
    off = np.array([0, 0, 5, 60, 60, 96, 112, 192, n, n], np.uint64)
    arr = np.frombuffer(text, np.uint8)
    rec, tid, first = oracle_batch_cut(o, arr, off)
    assert tid[rec["keyword_id"] == 4].tolist() == [2, 7] and o.scan(arr)["keyword_id"].tolist().count(4) == 3
    hits = np.diff(first.astype(np.int64)).astype(np.uint64)
    nontrivial(o, arr, off, hits)
    assert hits[5] == 0
    plan = m.plan(0)
    dev, d_off = _dev(torch_cuda, text), _dev(torch_cuda, off)
    for window in (16, 48, 4096):
        for invert in (False, True):
            want = expected(arr, off, hits, invert)
            g = plan.grep(dev, d_off, invert=invert, window=window, capacity=4096)
            assert 0 < g.need <= o.scan(arr).size
            check(_np(g, 1), hits, want, 1, (window, invert))
    for invert in (False, True):
        check(plan.grep_host(arr, off, invert=invert), hits, expected(arr, off, hits, invert), 1, "host")
    # an empty batch
    empty = _dev(torch_cuda, np.zeros(16, np.uint8))[:0]
    g = plan.grep(empty, _dev(torch_cuda, np.zeros(1, np.uint64)), window=16, capacity=64)
    assert (g.n_kept, g.total, g.need, g.out_symbols) == (0, 0, 0, 0) and g.hits.numel() == 0 and int(g.out_offsets[0].item()) == 0
    h = plan.grep_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert (h.n_kept, h.total, h.out_symbols) == (0, 0, 0) and h.out_offsets.tolist() == [0]
    # one text: the whole buffer
    one = np.array([0, n], np.uint64)
    hits1 = oracle_hits(o, arr, one)
    assert hits1.tolist() == [o.scan(arr).size]
    for window in (16, 4096):
        g = plan.grep(dev, _dev(torch_cuda, one), window=window, capacity=4096)
        check(_np(g, 1), hits1, expected(arr, one, hits1, False), 1, ("one text", window))
    # texts shorter than one window, one of them without a match
    short = [b"she", b"xyz", b"ushers hers"]
    sarr, soff = np.frombuffer(b"".join(short), np.uint8), offsets_of(short)
    shits = oracle_hits(o, sarr, soff)
    assert shits[1] == 0 and shits[0] > 0
    for invert in (False, True):
        g = plan.grep(_dev(torch_cuda, sarr), _dev(torch_cuda, soff), invert=invert, window=16, capacity=64)
        check(_np(g, 1), shits, expected(sarr, soff, shits, invert), 1, ("short", invert))
    plan.status()


def test_contention_and_overflow(torch_cuda, monkeypatch):
    text = np.frombuffer(b"a" * 65536, np.uint8)
    m, o = build_pair([b"a", b"aa", b"aaa"], 1)
    plan = m.plan(0)
    dev = _dev(torch_cuda, text)
    for off, want_hits in ((np.array([0, 65536], np.uint64), [196605]), (np.arange(5, dtype=np.uint64) * 16384, [49149] * 4)):
        hits = oracle_hits(o, text, off)
        assert hits.tolist() == want_hits
        d_off = _dev(torch_cuda, off)
        # 4,096 symbols x 3 records in a window of room for 4,096: nothing is reported but the need
        g = plan.grep(dev, d_off, window=4096, capacity=4096)
        assert g.need == 12288 > 4096 and g.n_kept == 0 and g.total == 0 and g.out_symbols == 0
        # the stated bound: window x M records cannot overflow; every add of a window on one address (or on two)
        g = plan.grep(dev, d_off, window=4096, capacity=12288)
        assert g.need == 12288
        check(_np(g, 1), hits, expected(text, off, hits, False), 1, "capacity 12288")
        g = plan.grep(dev, d_off, invert=True, window=4096, capacity=12288)
        check(_np(g, 1), hits, expected(text, off, hits, True), 1, "capacity 12288, inverted")
        # the host call with room for 4,096 records: the call repeats itself with windows of 4,096 / 3 symbols
        monkeypatch.setenv("ACM_GPU_TALLY_CAPACITY", "4096")
        check(plan.grep_host(text, off), hits, expected(text, off, hits, False), 1, "host, second attempt")
        monkeypatch.delenv("ACM_GPU_TALLY_CAPACITY")
    plan.status()


def small_dictionary(sb):
    """(keywords, alphabet) of a symbol size: four keywords over seven symbols with every byte set"""
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[sb]
    alphabet = (np.array([97, 98, 99, 100, 101, 102, 103], np.uint64) * np.uint64(int.from_bytes(b"\x01" * sb, "little"))).astype(dtype)
    return [alphabet[[0, 1, 2]], alphabet[[3, 3]], alphabet[[6, 5, 4, 3]], alphabet[[2, 0]]], alphabet


def _alignment_case(sb, monkeypatch, kat, small=False):
    """(oracle, plan maker, symbols, offsets) for a symbol size: the u64 kind, small dictionaries of our own
    otherwise (small: for 8-byte symbols too); one match of the buffer is copied across a text boundary"""
    rng = np.random.default_rng(40 + sb)
    lens = [0, 1, 15, 16, 17, 33] * 8 + [5000] + [33, 17, 16, 15, 1, 0] * 8
    n = sum(lens)
    if sb == 8 and not small:
        m, o, text, make_plan, plan_ok, form = kind("u64", monkeypatch, kat)
        base = text[1000:1000 + n].copy()
    else:
        kws, alphabet = small_dictionary(sb)
        m, o = build_pair(kws, sb)
        make_plan = m.plan
        base = alphabet[rng.integers(0, alphabet.size, size=n)]
    off = offsets_of([b"x" * k for k in lens])
    rec = o.scan(base)
    r = rec[rec["length"] >= 2][0]
    word = base[int(r["end_pos"]) + 1 - int(r["length"]):int(r["end_pos"]) + 1].copy()
    cut = int(off[5])                                                             # between the texts of 16 and of 17 symbols
    base[cut - 1:cut - 1 + word.size] = word
    return o, make_plan, base, off


@pytest.mark.parametrize("tile", [None, 256])
@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_gather_alignment(torch_cuda, monkeypatch, kat, sb, tile):
    """text and output each 0, 1, 7 and 15 symbols past a 16-byte boundary; texts of 0, 1, 15, 16, 17 and
    33 symbols and one of 5,000, so that a tile holds many boundaries and one text spans tiles (always
    with tiles of 256 bytes); guard bytes around the output"""
    if tile:
        monkeypatch.setenv("ACM_GPU_GREP_TILE", str(tile))
    o, make_plan, base, off = _alignment_case(sb, monkeypatch, kat)
    gather_alignment_on_plan(torch_cuda, make_plan(0), o, base, off, sb)


def gather_alignment_on_plan(torch_cuda, plan, o, base, off, sb):
    """test_gather_alignment's case through Plan.grep on a plan of the case's dictionary, however it came to hold it
    (tests/test_growth_gpu.py calls this with grown plans)"""
    hits = oracle_hits(o, base, off)
    nontrivial(o, base, off, hits)
    d_off = _dev(torch_cuda, off)
    shifts = sorted({(k * sb) % 16: k for k in (15, 7, 1, 0)}.values())
    pad = 64
    for invert in (False, True):
        want = expected(base, off, hits, invert)
        need = int(want[1][-1])
        for kt in shifts:
            dev = _off_at(torch_cuda, base, kt)
            for ko in shifts:
                for cap in (need, need - 1):
                    buf = torch_cuda.full((pad + ko * sb + need * sb + pad,), GUARD, dtype=torch_cuda.uint8, device="cuda")
                    out = buf[pad + ko * sb:pad + ko * sb + cap * sb]
                    assert out.data_ptr() % 16 == (ko * sb) % 16
                    g = plan.grep(dev, d_off, invert=invert, window=4096, capacity=1 << 15, out=out, out_capacity=cap)
                    got = _np(g, sb)
                    whole = buf.cpu().numpy()
                    assert np.all(whole[:pad + ko * sb] == GUARD) and np.all(whole[pad + ko * sb + cap * sb:] == GUARD), (kt, ko, cap)
                    if cap == need:
                        check(got, hits, want, sb, (invert, kt, ko))
                    else:                                                     # the need, everything but `out` still right
                        assert g.out_symbols == need > cap and got.out is None
                        check(got, hits, want, sb, (invert, kt, ko, "one short"))
        g = plan.grep(_dev(torch_cuda, base), d_off, invert=invert, window=4096, capacity=1 << 15, gather=False)
        assert g.out is None
        check(_np(g, sb), hits, want, sb, (invert, "no gather"))
    plan.status()


def test_grep_device_arguments_and_contract(torch_cuda):
    torch = torch_cuda
    m, o = build_pair([b"he", b"she"], 1)
    plan = m.plan(0)
    L = acm.lib()
    text = b"ushers" * 10
    dev = _dev(torch, text)
    n = dev.numel()
    off = np.array([0, 30, 30, n], np.uint64)
    d_off = _dev(torch, off)
    tb = L.acm_gpu_grep_tmp_bytes(plan.h, 16, 64, n, 3)
    assert tb >= 64 * 16 + 3 * 8
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    hits = torch.zeros(3, dtype=torch.int64, device="cuda")
    kept = torch.zeros(3, dtype=torch.int32, device="cuda")
    out_off = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    D = dict(n_texts=3, window=16, capacity=64, tmp_bytes=tb, d_out=out.data_ptr(), out_capacity=64, d_sym=res.data_ptr() + 24,
             d_nk=res.data_ptr(), d_total=res.data_ptr() + 8, d_need=res.data_ptr() + 16, offsets=d_off)

    def call(p=None, **kw):
        a = dict(D, **kw)
        return L.acm_gpu_grep_device((p or plan).h, dev.data_ptr(), n, a["offsets"].data_ptr(), a["n_texts"], 0, a["window"], a["capacity"],
                                     hits.data_ptr(), kept.data_ptr(), a["d_nk"], a["d_total"], a["d_need"], a["d_out"], a["out_capacity"],
                                     out_off.data_ptr(), a["d_sym"], tmp.data_ptr(), a["tmp_bytes"], None)
    assert call(window=0) == E_ARG and call(window=24) == E_ARG
    assert call(capacity=0) == E_ARG and call(capacity=1 << 31) == E_ARG
    assert call(tmp_bytes=tb - 1) == E_ARG and call(n_texts=1 << 31) == E_ARG
    assert call(d_out=dev.data_ptr() + 8, out_capacity=16) == E_ARG                      # the output inside the text
    assert call(d_sym=None) == E_ARG and call(d_out=None) == E_ARG                       # d_out_symbols is NULL iff d_out is
    assert call(d_nk=None) == E_ARG and call(d_total=None) == E_ARG and call(d_need=None) == E_ARG
    assert L.acm_gpu_grep_tmp_bytes(plan.h, 16, 0, n, 3) == 0 and L.acm_gpu_grep_tmp_bytes(plan.h, 16, 1 << 31, n, 3) == 0
    assert L.acm_gpu_grep_tmp_bytes(plan.h, 16, 64, n, 1 << 31) == 0
    torch.cuda.synchronize()
    assert not hits.cpu().numpy().any() and not out.cpu().numpy().any()
    assert call(window=64) == 0                                                          # one window
    torch.cuda.synchronize()
    want_hits = oracle_hits(o, np.frombuffer(text, np.uint8), off)
    assert want_hits.tolist() == [10, 0, 10] and hits.cpu().tolist() == [10, 0, 10] and res.cpu().tolist() == [2, 20, 20, 60]
    assert kept.cpu().tolist()[:2] == [0, 2] and out_off.cpu().tolist()[:3] == [0, 30, 60] and bytes(out.cpu().numpy()[:60]) == text
    plan.status()
    # offsets that break the contract, all of them inside the buffer's range: the error flag, all counts 0, no other output written
    for what, bad in (("decreasing", [0, 40, 30, n]), ("last", [0, 30, 30, n - 1]), ("first", [1, 30, 30, n])):
        fresh = m.plan(0)
        for t in (hits, kept, out_off, out):
            t.fill_(0x5A if t.dtype != torch.uint8 else GUARD)
        res.fill_(77)
        assert call(p=fresh, offsets=_dev(torch, np.array(bad, np.uint64))) == 0, what
        with pytest.raises(binding.ACMError) as e:
            fresh.status()
        assert e.value.code == -7, what
        got = res.cpu().tolist()
        assert got[0] == 0 and got[1] == 0 and got[3] == 0, (what, got)
        assert hits.cpu().tolist() == [0x5A] * 3 and kept.cpu().tolist() == [0x5A] * 3 and out_off.cpu().tolist() == [0x5A] * 4, what
        assert np.all(out.cpu().numpy() == GUARD), what
    plan.status()
