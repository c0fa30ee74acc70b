"""A buffer cut into texts on the GPU (acm_gpu_split_*, acm_gpu_grep_lines_host, acm_grep_lines;
csrc/dev_split.h).  Expected offsets always come from numpy on the caller's symbols
(tests/split_cases.py), expected hits from the ORACLE's scan of every text alone (tests/grep_cases.py);
every grep workload first shows from the oracle alone that it cannot pass trivially."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.cases import build_pair
from tests.grep_cases import check, expected, nontrivial, oracle_hits
from tests.split_cases import DELIM1, DELIM16, EDGES, expected_offsets, straddle, wide, with_delims
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind, novel_words

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD = -0x5A5A5A5A5A5A5A5B                                   # 0xA5A5A5A5A5A5A5A5 as an int64
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


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


def _sym(text, sb):
    """bytes -> an array of symbols of sb bytes (tests/split_cases.py::wide's symbols)"""
    return wide(text, sb).view(DTYPE[sb])


def _split(plan, dev, delims, runs):
    return plan.split(dev, delims, runs=runs).cpu().numpy().view(np.uint64)


_plans = {}


def _plan(sb, monkeypatch, kat):
    """a plan of the symbol size, made once: the dense, the start-parallel and the interned 8-byte kind of
    tests/tally_cases.py; no kind has 2-byte symbols, so a small dictionary of our own there"""
    if sb not in _plans:
        if sb == 2:
            m, o = build_pair([np.array([104, 101], np.uint16), np.array([115], np.uint16)], 2)
            _plans[sb] = (m, m.plan(0))
        else:
            m, o, text, make_plan, plan_ok, form = kind({1: "dense", 4: "starts", 8: "u64"}[sb], monkeypatch, kat)
            plan = make_plan(0)
            assert plan_ok(plan) and plan.sym_size == sb
            _plans[sb] = (m, plan)
    return _plans[sb][1]


def _edge_buffers(novel_bytes, sb, runs):
    """(what, bytes, delimiters): every buffer is given as letters, one per symbol"""
    T = 256 // sb                                              # symbols per tile of 256 bytes
    W = 16 // sb                                               # symbols per 16-byte word
    cases = [("edge %r" % e, with_delims(e, d), d) for e in EDGES for d in (DELIM1, DELIM16)]
    prose = novel_bytes[3000:3000 + 4 * 256 + 16]
    for b in (255, 256, 257, 3 * 256 + 1):
        for n in sorted({b // sb, b // sb + 1}):
            cases.append(("%d bytes: %d symbols" % (b, n), prose[:n], b" \n"))
            cases.append(("%d bytes: %d symbols, 16 delimiters" % (b, n), prose[:n], DELIM16))
    flat = b"a" * (3 * T)

    def put(at, text=flat):
        t = bytearray(text)
        for i in at:
            t[i] = 10
        return bytes(t)
    cases += [("last of a tile", put([T - 1]), DELIM1), ("first of the next", put([T]), DELIM1), ("last and first", put([T - 1, T]), DELIM1),
              ("last of the second tile and all around", put([2 * T - 2, 2 * T - 1, 2 * T, 2 * T + 1]), DELIM1)]
    if runs:
        cases += [("a run across a tile boundary", put(range(T - 3, T + 3)), DELIM1),
                  ("a run across a word boundary", put(range(W - 1, W + 1)) if W > 1 else put([0, 1]), DELIM1),
                  ("a run across three words", put(range(2 * W - 1, 4 * W + 1)), DELIM1),
                  ("a run that ends the buffer", put(range(3 * T - 5, 3 * T)), DELIM1),
                  ("a run that ends the buffer in the next tile's first word", put(range(2 * T - 2, 2 * T + 1), flat[:2 * T + 1]), DELIM1)]
    return cases


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
@pytest.mark.parametrize("runs", [False, True])
def test_edges_with_tiles_of_256_bytes(torch_cuda, monkeypatch, kat, novel_bytes, sb, runs):
    monkeypatch.setenv("ACM_GPU_SPLIT_TILE", "256")
    plan = _plan(sb, monkeypatch, kat)
    for what, text, delims in _edge_buffers(novel_bytes, sb, runs):
        sym, d = _sym(text, sb), _sym(delims, sb)
        want = expected_offsets(sym, d, runs)
        dev = _dev(torch_cuda, sym) if sym.size else _dev(torch_cuda, np.zeros(16, DTYPE[sb]))[:0]
        got = _split(plan, dev, d, runs)
        assert np.array_equal(got, want), (what, got[:8], want[:8], got.size, want.size)
        assert np.array_equal(plan.split_host(sym, d, runs=runs), want), (what, "host")
    plan.status()


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_alignment_and_what_lies_outside_the_buffer(torch_cuda, monkeypatch, kat, novel_bytes, sb):
    """the text k symbols past a 16-byte boundary, for every k; the bytes in front of it and behind it (the
    rest of its first and last aligned word and a word more) all hold the delimiter and must not count"""
    plan = _plan(sb, monkeypatch, kat)
    per = 16 // sb
    d = _sym(b"\n", sb)
    for tile in (None, 256):
        if tile:
            monkeypatch.setenv("ACM_GPU_SPLIT_TILE", str(tile))
        for k in range(1, per):
            for n in (999, 1000 - k, 2 * per - k + 1):
                body = bytearray(novel_bytes[5000:5000 + n])                  # neither end a delimiter, one in between
                body[0], body[-1], body[n // 2] = 122, 122, 10
                sym = _sym(body, sb)
                whole = _dev(torch_cuda, np.concatenate([np.repeat(d, k), sym, np.repeat(d, 2 * per)]))
                dev = whole[k:k + n]
                assert dev.data_ptr() % 16 == k * sb and dev.is_contiguous()
                for runs in (False, True):
                    want = expected_offsets(sym, d, runs)
                    got = _split(plan, dev, d, runs)
                    assert np.array_equal(got, want), (tile, k, n, runs, got[:4], want[:4], got[-3:], want[-3:])
    # the delimiter's bytes across two symbols are no delimiter
    if sb > 1:
        text, delim = straddle(sb)
        longer = np.concatenate([text, text[:2], np.array([0x41], text.dtype)])
        for runs in (False, True):
            assert _split(plan, _dev(torch_cuda, text), delim, runs).tolist() == [0, 3]
            assert _split(plan, _dev(torch_cuda, longer), delim, runs).tolist() == [0, 3, 6]
            assert _split(plan, _off_at(torch_cuda, longer, 1), delim, runs).tolist() == [0, 3, 6]
    plan.status()


@pytest.mark.parametrize("runs", [False, True])
def test_capacity_count_only_exact_and_one_short(torch_cuda, monkeypatch, kat, novel_bytes, runs):
    torch = torch_cuda
    monkeypatch.setenv("ACM_GPU_SPLIT_TILE", "256")
    plan = _plan(1, monkeypatch, kat)
    L = acm.lib()
    text = np.frombuffer(novel_bytes[:5000], np.uint8)
    d = np.frombuffer(b" \n", np.uint8)
    want = expected_offsets(text, d, runs)
    need = want.size - 1
    dev = _dev(torch, text)
    tb = L.acm_gpu_split_tmp_bytes(plan.h, text.size)
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    pad = 8

    def call(cap, offsets=True):
        buf = torch.full((pad + cap + 1 + pad,), GUARD, dtype=torch.int64, device="cuda")
        rc = L.acm_gpu_split_device(plan.h, dev.data_ptr(), text.size, d.ctypes.data, d.size, int(runs), buf.data_ptr() + 8 * pad if offsets else None,
                                    cap, count.data_ptr(), tmp.data_ptr(), tb, None)
        assert rc == 0
        torch.cuda.synchronize()
        return int(count.item()), buf.cpu().numpy()
    n, buf = call(0, offsets=False)                            # count only: the capacity is ignored
    assert n == need and np.all(buf == GUARD)
    n, buf = call(need)                                        # exactly
    assert n == need and np.array_equal(buf[pad:pad + need + 1].view(np.uint64), want)
    assert np.all(buf[:pad] == GUARD) and np.all(buf[pad + need + 1:] == GUARD)
    n, buf = call(need - 1)                                    # one short: the need, nothing outside offsets[0 .. capacity]
    assert n == need > need - 1
    assert np.all(buf[:pad] == GUARD) and np.all(buf[pad + need:] == GUARD)
    n, buf = call(3)
    assert n == need and np.all(buf[:pad] == GUARD) and np.all(buf[pad + 4:] == GUARD)
    with pytest.raises(binding.ACMError) as e:
        plan.split(dev, d, runs=runs, capacity=need - 1)
    assert e.value.code == E_OVERFLOW and e.value.need == need
    assert np.array_equal(plan.split(dev, d, runs=runs, capacity=need + 5).cpu().numpy().view(np.uint64), want)
    with pytest.raises(binding.ACMError) as e:
        plan.split_host(text, d, runs=runs, capacity=need - 1)
    assert e.value.code == E_OVERFLOW and e.value.need == need
    plan.status()


def test_workload_the_novel_as_lines_and_as_words(torch_cuda, monkeypatch, kat, novel_bytes):
    plan = _plan(1, monkeypatch, kat)
    novel = np.frombuffer(novel_bytes, np.uint8)
    assert novel.size == 376617 and np.count_nonzero(novel == 10) == 5999 and novel[-1] == 10
    nl, blank = np.frombuffer(b"\n", np.uint8), np.frombuffer(b" \t\n", np.uint8)
    lines = expected_offsets(novel, nl, False)
    assert lines.size - 1 == 5999 and np.count_nonzero(np.diff(lines.astype(np.int64)) == 1) == 906
    cut = novel[:-2]
    assert cut[-1] != 10 and expected_offsets(cut, nl, False).size - 1 == np.count_nonzero(cut == 10) + 1   # the unterminated last line is a text
    words = expected_offsets(novel, blank, True)
    assert words.size - 1 == 63557 + 1 and novel[0] in blank                     # 63,557 words, and the run of delimiters the novel begins with
    for tile in (None, 256):
        if tile:
            monkeypatch.setenv("ACM_GPU_SPLIT_TILE", str(tile))
        for what, text, d, runs, want in (("lines", novel, nl, False, lines), ("unterminated", cut, nl, False, expected_offsets(cut, nl, False)),
                                          ("words", novel, blank, True, words), ("lines as runs", novel, nl, True, expected_offsets(novel, nl, True))):
            got = _split(plan, _dev(torch_cuda, text), d, runs)
            assert np.array_equal(got, want), (tile, what, got.size, want.size)
    plan.status()


def test_composition_split_offsets_feed_the_batch_calls(torch_cuda, novel_bytes):
    m, o = build_pair(novel_words(novel_bytes, 200), 1)
    plan = m.plan(0)
    novel = np.frombuffer(novel_bytes, np.uint8)
    dev = _dev(torch_cuda, novel)
    made = _dev(torch_cuda, expected_offsets(novel, np.frombuffer(b"\n", np.uint8), False))
    split = plan.split(dev)
    assert split.dtype == made.dtype and split.shape == made.shape and split.is_contiguous()
    a, b = _np(plan.grep(dev, split), 1), _np(plan.grep(dev, made), 1)
    assert a.n_kept == b.n_kept > 0 and a.total == b.total > 0
    for field in ("hits", "kept", "out_offsets", "out"):
        assert np.array_equal(getattr(a, field), getattr(b, field)), field
    for x, y, what in zip(plan.scan_batch(dev, split), plan.scan_batch(dev, made), ("records", "text_id", "first")):
        assert x.shape == y.shape and x.size and np.array_equal(x, y), what
    ta, tb = plan.tally_batch(dev, split), plan.tally_batch(dev, made)
    assert ta.nnz == tb.nnz > 0 and ta.total == tb.total == a.total
    for field in ("row_ptr", "col", "val"):
        x, y = getattr(ta, field).cpu().numpy(), getattr(tb, field).cpu().numpy()
        assert np.array_equal(x[:ta.nnz] if field != "row_ptr" else x, y[:tb.nnz] if field != "row_ptr" else y), field
    plan.status()


def _lines_case(name, monkeypatch, kat, novel_bytes):
    """(machine, oracle, text, plan maker, plan check, delimiters, offsets, oracle hits) of a plan kind.
    The novel is cut at its newlines; a kind's own text gets a delimiter value of its own planted every
    37th to 97th symbol.  The oracle then shows, here on the CPU, whether the texts have two distinct
    non-zero hit counts and whether a match of the whole buffer crosses a boundary.  No keyword holds
    such a delimiter, so none does; and a delimiter WRITTEN into a match would take the match out of the
    whole buffer as well.  So the cuts inside matches are made the other way round: of the symbols in
    front of the last one of five matches of three symbols or more, the one the text holds least often
    becomes a second delimiter, which cuts that match, and every other one that holds the symbol, in two
    (and leaves the texts long enough for some to have more than one match)."""
    m, o, text, make_plan, plan_ok, form = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
        delims = [10]
    else:
        text = text[:200000].copy()
        planted = int(text.max()) + 1
        rng = np.random.default_rng(11)
        at = np.cumsum(rng.integers(37, 98, size=text.size // 37))
        text[at[at < text.size]] = planted
        delims = [planted]
    whole = o.scan(text)
    off = expected_offsets(text, np.array(delims, text.dtype), False)
    hits = oracle_hits(o, text, off)
    if not (np.unique(hits[hits > 0]).size >= 2 and whole.size > int(hits.sum())):
        long_ones = whole[whole["length"] >= 3]
        inside = long_ones["end_pos"][:: max(long_ones.size // 5, 1)][:5].astype(np.int64) - 1
        delims.append(min((int(x) for x in text[inside]), key=lambda x: int(np.count_nonzero(text == x))))
    return m, o, text, make_plan, plan_ok, np.array(delims, text.dtype)


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind_three_entry_points(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram, CSR (a dense plan on a pointer off the 16-byte grid), start-parallel, sparse walk,
    8-byte symbols, comparator classes, a plan with a pending delta -- through Plan.split + Plan.grep,
    Plan.grep_lines_host and Machine.grep_lines, with both grep flags"""
    m, o, text, make_plan, plan_ok, delims = _lines_case(name, monkeypatch, kat, novel_bytes)
    sb = text.itemsize
    plan = make_plan(0)                                        # (the delta kind's maker also completes the oracle's dictionary)
    assert plan_ok(plan), plan.describe()
    off = expected_offsets(text, delims, False)
    hits = oracle_hits(o, text, off)
    print("%s: %d symbols, %d delimiters, %d texts" % (name, text.size, delims.size, off.size - 1))
    nontrivial(o, text, off, hits)
    dev = _off_at(torch_cuda, text, 1 if name == "csr" else 0)
    split = plan.split(dev, delims)
    assert np.array_equal(split.cpu().numpy().view(np.uint64), off)
    for invert in (False, True):
        want = expected(text, off, hits, invert)
        check(_np(plan.grep(dev, split, invert=invert), sb), hits, want, sb, "%s Plan.split + Plan.grep invert=%d" % (name, invert))
        plan.status()
        for what, g in (("Plan.grep_lines_host", plan.grep_lines_host(text, delims, invert=invert)),
                        ("Machine.grep_lines", m.grep_lines(text, delims, invert=invert))):
            assert g.n_texts == off.size - 1 and np.array_equal(g.offsets, off), (name, what)
            check(g, hits, want, sb, "%s %s invert=%d" % (name, what, invert))
        assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    g = plan.grep_lines_host(text, delims, gather=False)
    assert g.out is None
    check(g, hits, expected(text, off, hits, False), sb, "no gather")
    if name == "classes":
        # the delimiter is matched on the caller's symbols: under the case-folding comparator "X" is no cut
        small = np.frombuffer(b"aXbxcXdx He", np.uint8)
        assert plan.split(_dev(torch_cuda, small), b"x").cpu().tolist() == [0, 4, 8, 11]
        g = plan.grep_lines_host(small, b"x")
        assert g.offsets.tolist() == [0, 4, 8, 11] and g.hits.tolist() == [0, 0, 1]
    # words
    runs_off = expected_offsets(text, delims, True)
    assert np.array_equal(plan.grep_lines_host(text, delims, runs=True, gather=False).offsets, runs_off)
    plan.status()


def test_split_device_arguments(torch_cuda, monkeypatch, kat):
    torch = torch_cuda
    plan1, plan4 = _plan(1, monkeypatch, kat), _plan(4, monkeypatch, kat)
    L = acm.lib()
    text = _dev(torch, b"ab\ncd\nef" * 8)
    n = text.numel()
    d = np.frombuffer(b"\n" * 17, np.uint8)
    d4 = np.array([10], np.uint32)
    tb = L.acm_gpu_split_tmp_bytes(plan1.h, n)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    off = torch.full((64,), GUARD, dtype=torch.int64, device="cuda")
    count = torch.full((1,), 77, dtype=torch.int64, device="cuda")

    def call(plan=plan1, ptr=text.data_ptr(), n_symbols=n, delims=d.ctypes.data, n_delims=1, flags=0, offsets=off.data_ptr(), capacity=32,
             d_n=count.data_ptr(), tmp_bytes=tb):
        return L.acm_gpu_split_device(plan.h if plan else None, ptr, n_symbols, delims, n_delims, flags, offsets, capacity, d_n, tmp.data_ptr(),
                                      tmp_bytes, None)
    assert call(n_delims=0) == E_ARG and call(n_delims=17) == E_ARG and call(flags=2) == E_ARG
    assert call(capacity=1 << 31) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(plan=None) == E_ARG
    assert call(d_n=None) == E_ARG and call(delims=None) == E_ARG
    assert call(plan=plan4, ptr=text.data_ptr() + 2, n_symbols=4, delims=d4.ctypes.data) == E_ARG       # no multiple of the symbol size
    torch.cuda.synchronize()
    assert int(count.item()) == 77 and np.all(off.cpu().numpy() == GUARD)
    assert call(n_delims=16) == 0 and call(capacity=(1 << 31) - 1) == 0
    assert call(offsets=None, capacity=1 << 40) == 0                                                  # count only: the capacity is ignored
    torch.cuda.synchronize()
    assert int(count.item()) == 17                                                                    # 16 newlines and the unterminated rest
    # no symbol: no text, offsets = [0]
    assert call(n_symbols=0) == 0
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and int(off[0].item()) == 0
    empty = _dev(torch, np.zeros(16, np.uint8))[:0]
    assert plan1.split(empty).cpu().tolist() == [0] and plan1.split_host(np.zeros(0, np.uint8)).tolist() == [0]
    g = plan1.grep_lines_host(np.zeros(0, np.uint8))
    assert (g.n_texts, g.n_kept, g.total, g.out_symbols) == (0, 0, 0, 0) and g.offsets.tolist() == [0]
    assert L.acm_gpu_split_tmp_bytes(plan1.h, 1 << 62) == 0
    plan1.status()
    plan4.status()
