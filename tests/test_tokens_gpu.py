"""Tokenising on the GPU (acm_gpu_tokens_*, acm_gpu_scan_tokens_*, acm_tokenize; csrc/dev_tokens.h).
The expected stream is always the definition in plain Python over select_cases.greedy of the ORACLE's
records (tests/token_cases.py) -- per text via batch_cases.oracle_batch for batches --, never the
library's own scan or selection; every workload case first shows from the oracle alone that a record
is selected, a record is left out, a gap token exists and, for batches, that a run is cut by a text
boundary and a text is empty.  Every output lies between canaries."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, random_cuts
from tests.cases import build_pair, rand_words
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind
from tests.token_cases import DROP, MODES, RUN, SYMBOL, oracle_case, selection_of, tokens_by_definition

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
GUARD = 64
TILES = ["64", None]                                     # ACM_GPU_TOKENS_TILE: the smallest, and the default (8,192)
GB = 1 << 20


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _tile(monkeypatch, tile):
    monkeypatch.delenv("ACM_GPU_TOKENS_TILE", raising=False)
    if tile is not None:
        monkeypatch.setenv("ACM_GPU_TOKENS_TILE", tile)


def _bytes_of(arr):
    return np.frombuffer(bytes(arr), np.uint8) if isinstance(arr, (bytes, bytearray)) else np.ascontiguousarray(arr).view(np.uint8).reshape(-1)


def _dev(torch, arr, at=0):
    """the bytes of `arr` on the device, beginning `at` bytes behind a 256-byte boundary"""
    b = _bytes_of(arr)
    buf = torch.zeros(at + b.size + 16, dtype=torch.uint8, device="cuda")
    buf[at:at + b.size] = torch.from_numpy(b.copy()).cuda()
    view = buf[at:at + b.size]
    assert view.data_ptr() % 16 == at % 16 and view.is_contiguous()
    return view


class _Out:
    """an output array of n entries with GUARD canary entries in front and behind"""

    def __init__(self, torch, n, dtype):
        self.canary = 0x5A5A5A5A if dtype == torch.int32 else 0x5A5A5A5A5A5A5A5A
        self.whole = torch.full((GUARD + n + GUARD,), self.canary, dtype=dtype, device="cuda")
        self.view = self.whole[GUARD:GUARD + n]
        self.n = n
        self.np_dtype = np.uint32 if dtype == torch.int32 else np.uint64

    def canaries_intact(self):
        w = self.whole.cpu().numpy()
        return bool(np.all(w[:GUARD] == self.canary) and np.all(w[GUARD + self.n:] == self.canary))

    def untouched(self):
        return bool(np.all(self.whole.cpu().numpy() == self.canary))

    def host(self, k):
        return self.whole.cpu().numpy()[GUARD:GUARD + k].view(self.np_dtype).copy()


class _Result:
    pass


def _outputs(torch, tok_cap, n_first):
    r = _Result()
    r.ids, r.start, r.length = _Out(torch, tok_cap, torch.int32), _Out(torch, tok_cap, torch.int64), _Out(torch, tok_cap, torch.int32)
    r.first = _Out(torch, n_first, torch.int64) if n_first else None
    r.res = torch.full((2,), 0x5A5A, dtype=torch.int64, device="cuda")
    return r


def _scan(torch, plan, text, off, mode, rec_cap, tok_cap, gap_base=GB, tok_of=None, text_at=0, pos_base=0, count_only=False, n_symbols=None):
    """acm_gpu_scan_tokens_device itself, every output between canaries: a _Result with count, n_tokens"""
    L = acm.lib()
    sb = plan.sym_size
    d_text = _dev(torch, text, text_at)
    n_sym = _bytes_of(text).size // sb if n_symbols is None else n_symbols
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda() if off is not None else None
    n_texts = len(off) - 1 if off is not None else 0
    r = _outputs(torch, tok_cap, len(off) if off is not None else 0)
    r.records = torch.zeros((max(rec_cap, 1), 2), dtype=torch.int64, device="cuda")
    d_of = torch.from_numpy(np.asarray(tok_of, np.uint32).view(np.int32).copy()).cuda() if tok_of is not None else None
    tb = L.acm_gpu_scan_tokens_tmp_bytes(plan.h, rec_cap, n_sym, n_texts)
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_scan_tokens_device(plan.h, d_text.data_ptr(), n_sym, pos_base, d_off.data_ptr() if d_off is not None else None, n_texts,
                                      r.records.data_ptr(), rec_cap, r.res.data_ptr(), d_of.data_ptr() if d_of is not None else None,
                                      len(tok_of) if tok_of is not None else 0, gap_base, mode,
                                      None if count_only else r.ids.view.data_ptr(), None if count_only else r.start.view.data_ptr(),
                                      None if count_only else r.length.view.data_ptr(), tok_cap, r.res.data_ptr() + 8,
                                      r.first.view.data_ptr() if r.first is not None else None, tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    r.count, r.n_tokens = (int(x) for x in r.res.cpu())
    return r


def _assert_stream(r, want, n_symbols=None, mode=None):
    ids, starts, lens, first = want
    n = ids.size
    assert r.n_tokens == n, (r.n_tokens, n)
    if r.first is not None:
        got = r.first.host(first.size)
        bad = np.flatnonzero(got != first)
        assert bad.size == 0, ("tok_first", bad[:8], got[bad[:8]], first[bad[:8]])
        assert r.first.canaries_intact() and got[0] == 0 and got[-1] == n
    for name, out, exp in (("tok_start", r.start, starts), ("tok_len", r.length, lens), ("tok_id", r.ids, ids)):
        got = out.host(n)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], exp[bad[:8]])
        assert out.canaries_intact(), name
    got = r.start.host(n)
    assert np.all(got[1:] > got[:-1])                                        # starts ascend strictly
    if n_symbols is not None and mode != DROP:
        assert int(r.length.host(n).astype(np.int64).sum()) == n_symbols     # the tokens tile the buffer


def _check(torch, plan, text, rec, sel, off, mode, gap_base=GB, tok_of=None, text_at=0, pos_base=0, want=None, cap=None):
    """acm_gpu_scan_tokens_device with exactly the room the records and the tokens need.  `cap`: for a
    batch the record room holds the matches of the whole buffer (the batch scan's rule), the oracle's
    count of the buffer as one text"""
    if want is None:
        shifted = sel.copy()
        shifted["end_pos"] += np.uint64(pos_base)
        want = tokens_by_definition(text, shifted, mode, gap_base, tok_of, off, pos_base)
    r = _scan(torch, plan, text, off, mode, max(rec.size if cap is None else cap, 1), want[0].size, gap_base, tok_of, text_at, pos_base)
    assert r.count == sel.size, (r.count, sel.size)
    _assert_stream(r, want, _bytes_of(text).size // plan.sym_size, mode)
    got = np.frombuffer(r.records[:r.count].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE)
    shifted = sel.copy()
    shifted["end_pos"] += np.uint64(pos_base)
    assert np.array_equal(got, shifted)                                      # the selected records stay in d_records
    plan.status()
    return r


# ---- 1. tile edges, at the smallest tile
def _edge_text():
    """832 symbols = 13 tiles of 64: `needle` at 0, across the tile edge at 64 (61 .. 66) and at the end;
    q's from 67 to 299, cut by the text boundary on the tile edge at 128 and by the two empty texts on
    the tile edge at 192; q's from 506 to 825, one run over six tiles; `dle` inside every needle is the
    record left out"""
    n = 832
    text = np.full(n, ord("q"), np.uint8)
    for at in (0, 61, 300, 500, n - 6):
        text[at:at + 6] = np.frombuffer(b"needle", np.uint8)
    text[400:403] = np.frombuffer(b"dle", np.uint8)
    off = np.array([0, 0, 128, 192, 192, 192, 450, n, n], np.uint64)
    return text, off


@pytest.mark.parametrize("mode", MODES)
def test_tile_edges(torch_cuda, monkeypatch, mode):
    _tile(monkeypatch, "64")
    text, off = _edge_text()
    m, o = build_pair([b"needle", b"dle"], 1)
    plan = m.plan(0)
    rec, sel = oracle_case(o, text, off)
    starts = sel["end_pos"].astype(np.int64) + 1 - sel["length"].astype(np.int64)
    assert starts[0] == 0 and int(sel[-1]["end_pos"]) == text.size - 1       # a match at symbol 0 and one that ends at n - 1
    assert np.any((starts < 64) & (sel["end_pos"].astype(np.int64) >= 64))   # a selected match across a tile edge
    want = tokens_by_definition(text, sel, mode, GB, None, off)
    if mode == RUN:                                                          # the runs cut on the tile edges, and the run over six tiles
        k = int(np.flatnonzero(want[1] == 128)[0])
        assert (want[1][k - 1], want[2][k - 1]) == (67, 61) and want[2][k] == 64 and (want[1][k + 1], want[2][k + 1]) == (192, 108)
        assert want[2][int(np.flatnonzero(want[1] == 506)[0])] == 320
        assert want[3].tolist()[2:6] == [k, k + 1, k + 1, k + 1]             # the rank at a boundary on a tile edge, for the empty texts too
    rec1, sel1 = oracle_case(o, text)                                        # the same buffer as one text
    _check(torch_cuda, plan, text, rec, sel, off, mode, want=want, cap=rec1.size)
    _check(torch_cuda, plan, text, rec1, sel1, None, mode)
    # a buffer with no record at all, as a batch and as one text
    quiet = np.full(300, ord("q"), np.uint8)
    qoff = np.array([0, 64, 64, 130, 300], np.uint64)
    none = np.zeros(0, po.RECORD_DTYPE)
    r = _check(torch_cuda, plan, quiet, none, none, qoff, mode)
    assert r.n_tokens == {SYMBOL: 300, RUN: 3, DROP: 0}[mode]
    r = _check(torch_cuda, plan, quiet, none, none, None, mode)
    assert r.n_tokens == {SYMBOL: 300, RUN: 1, DROP: 0}[mode]
    # n = 0: no token, every tok_first is 0
    r = _scan(torch_cuda, plan, np.zeros(16, np.uint8), np.array([0, 0, 0], np.uint64), mode, 4, 4, n_symbols=0)
    assert (r.count, r.n_tokens) == (0, 0) and r.first.host(3).tolist() == [0, 0, 0] and r.first.canaries_intact()
    assert r.ids.untouched() and r.start.untouched() and r.length.untouched()
    r = _scan(torch_cuda, plan, np.zeros(16, np.uint8), None, mode, 4, 4, n_symbols=0)
    assert (r.count, r.n_tokens) == (0, 0) and r.ids.untouched()
    plan.status()


# ---- 2. the novel, split into lines
@pytest.fixture(scope="module")
def novel_case(novel_bytes):
    """the first 64 Ki symbols, cut behind every newline by numpy; the buffer's end is listed twice, so
    that the batch ends with an empty text"""
    text = np.frombuffer(novel_bytes, np.uint8)[:1 << 16].copy()
    cuts = np.flatnonzero(text == 10) + 1
    off = np.concatenate([[0], cuts[cuts < text.size], [text.size, text.size]]).astype(np.uint64)
    m, o = build_pair(KEYWORDS, 1)
    rec, sel = oracle_case(o, text, off)
    want = {mode: tokens_by_definition(text, sel, mode, GB, None, off) for mode in MODES}
    want["cap"] = selection_of(o, text)[0].size                              # the matches of the buffer as one text: the record room of a batch
    return m, text, off, rec, sel, want


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("mode", MODES)
def test_the_novel_line_by_line(torch_cuda, monkeypatch, novel_case, tile, mode):
    _tile(monkeypatch, tile)
    m, text, off, rec, sel, want = novel_case
    assert off.size > 500
    _check(torch_cuda, m.plan(0), text, rec, sel, off, mode, want=want[mode], cap=want["cap"])


# ---- 3. plan kinds and symbol sizes
def _overlap_across_the_delta(text):
    """a keyword of the plan's own tables (the first 300 of 450) written into the text with a keyword of
    the delta (300 .. 448) beginning on its last symbol: one record of each overlap, and the selection
    drops the delta's (tests/test_select_gpu.py has the same case)"""
    kd, ko = acm.synth.keywords(450)
    a, b = next((a, b) for a in range(300) for b in range(300, 449) if kd[ko[a + 1] - 1] == kd[ko[b]] and ko[b + 1] - ko[b] > 1)
    both = np.concatenate([kd[ko[a]:ko[a + 1]], kd[ko[b] + 1:ko[b + 1]]])
    text[50_000:50_000 + both.size] = both
    return text


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind(torch_cuda, monkeypatch, kat, novel_bytes, name, tile):
    torch = torch_cuda
    _tile(monkeypatch, tile)
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    text = text[:1 << 16].copy()
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    if name == "csr":
        text = text[1:]
    if name == "delta":
        text = _overlap_across_the_delta(text)
    off = random_cuts(text.size, 64, seed=len(name))
    rec, sel = oracle_case(o, text, off)
    tok_of = (np.arange(o.nb_keywords, dtype=np.uint32) * 7 + 3)
    rec1, sel1 = oracle_case(o, text)
    _check(torch, plan, text, rec, sel, off, RUN, tok_of=tok_of, text_at=1 if name == "csr" else 0, cap=rec1.size)
    _check(torch, plan, text, rec1, sel1, None, DROP, text_at=1 if name == "csr" else 0)
    if text.dtype.itemsize == 1:                                             # SYMBOL mode: symbols of 1 and 2 bytes only
        want = tokens_by_definition(text, sel, SYMBOL, GB, tok_of, off)
        if name == "classes":                                                # the gap ids are the caller's own symbols: Mrs / mrs / MRS are one class
            unc = want[0][(want[2] == 1) & (want[0] >= GB)] - GB
            assert np.any((unc >= ord("A")) & (unc <= ord("Z"))) and np.any((unc >= ord("a")) & (unc <= ord("z")))
            lower = tokens_by_definition(np.frombuffer(bytes(text).lower(), np.uint8), sel, SYMBOL, GB, tok_of, off)
            assert not np.array_equal(lower[0], want[0])
        _check(torch, plan, text, rec, sel, off, SYMBOL, tok_of=tok_of, text_at=1 if name == "csr" else 0, want=want, cap=rec1.size)
    else:
        r_cap = max(rec.size, 1)
        L = acm.lib()
        res = torch.zeros(2, dtype=torch.int64, device="cuda")
        tmp = torch.empty(L.acm_gpu_scan_tokens_tmp_bytes(plan.h, r_cap, text.size, 0), dtype=torch.uint8, device="cuda")
        recs = torch.zeros((r_cap, 2), dtype=torch.int64, device="cuda")
        rc = L.acm_gpu_scan_tokens_device(plan.h, _dev(torch, text).data_ptr(), text.size, 0, None, 0, recs.data_ptr(), r_cap, res.data_ptr(), None, 0,
                                          0, SYMBOL, None, None, None, 0, res.data_ptr() + 8, None, tmp.data_ptr(), tmp.numel(), None)
        assert rc == E_ARG                                                   # no byte fallback for symbols of 4 and 8 bytes
    if name == "delta":                                                      # a table without the delta's keywords
        assert plan.tally_keywords == o.nb_keywords == 450 and int(sel["keyword_id"].max()) >= 300
        with pytest.raises(acm.ACMError) as e:
            plan.scan_tokens(_dev(torch, text), tok_of=tok_of[:300], capacity=rec1.size)
        assert e.value.code == E_ARG
        with pytest.raises(acm.ACMError) as e:
            plan.scan_tokens_host(text, tok_of=tok_of[:449])
        assert e.value.code == E_ARG
    texts = [text[int(off[t]):int(off[t + 1])] for t in range(off.size - 1)]
    tok = m.tokenize(texts, mode="run", gap_base=GB, tok_of=tok_of)
    want = tokens_by_definition(text, sel, RUN, GB, tok_of, off)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    assert tok.n_tokens == want[0].size and tok.count == sel.size
    assert np.array_equal(tok.ids, want[0]) and np.array_equal(tok.start, want[1]) and np.array_equal(tok.length, want[2])
    assert np.array_equal(tok.first, want[3])


@pytest.mark.parametrize("tile", TILES)
def test_two_byte_symbols(torch_cuda, monkeypatch, tile):
    _tile(monkeypatch, tile)
    rng = np.random.default_rng(1234)
    keywords = rand_words(rng, 200, 0, 600, 1, 5, np.uint16)
    text = rng.integers(0, 600, size=30001).astype(np.uint16)
    text[::97] = 0xFFFF                                                      # the greatest value: gap_base + 65535 = 2^32 - 1
    m, o = build_pair(keywords, 2)
    plan = m.plan(0)
    assert plan.info.kernel == 4, plan.describe()                            # the start-parallel scan
    off = random_cuts(text.size, 64, seed=2)
    rec, sel = oracle_case(o, text, off)
    gb = (1 << 32) - (1 << 16)
    want = tokens_by_definition(text, sel, SYMBOL, gb, None, off)
    assert int(want[0].max()) == (1 << 32) - 1
    cap = selection_of(o, text)[0].size
    _check(torch_cuda, plan, text, rec, sel, off, SYMBOL, gap_base=gb, text_at=2, want=want, cap=cap)
    _check(torch_cuda, plan, text, rec, sel, off, RUN, gap_base=gb, cap=cap)
    tok = plan.scan_tokens_host(text, off, mode="symbol", gap_base=gb)
    assert np.array_equal(tok.ids, want[0]) and np.array_equal(tok.first, want[3])
    with pytest.raises(acm.ACMError) as e:                                   # gap_base one too large
        plan.scan_tokens(_dev(torch_cuda, text), mode="symbol", gap_base=gb + 1, capacity=rec.size)
    assert e.value.code == E_ARG


# ---- 4. SYMBOL mode with the text 0, 1, 3 and 8 bytes behind a 16-byte boundary
@pytest.mark.parametrize("tile", TILES)
def test_symbol_mode_text_alignments(torch_cuda, monkeypatch, novel_case, tile):
    _tile(monkeypatch, tile)
    m, text, off, rec, sel, want = novel_case
    text, off = text[:20011], None
    rec, sel = oracle_case(build_pair(KEYWORDS, 1)[1], text)
    want = tokens_by_definition(text, sel, SYMBOL, 5)
    plan = m.plan(0)
    for at in (0, 1, 3, 8):
        _check(torch_cuda, plan, text, rec, sel, None, SYMBOL, gap_base=5, text_at=at, want=want)


def test_nonzero_pos_base(torch_cuda):
    text = b"To ushers: he found his pencil, but she could not find hers." * 20
    m, o = build_pair([b"he", b"she", b"his", b"hers"], 1)
    rec, sel = oracle_case(o, text)
    for mode in MODES:
        r = _check(torch_cuda, m.plan(0), text, rec, sel, None, mode, pos_base=(1 << 33) + 5, text_at=3)
        assert int(r.start.host(1)[0]) >= (1 << 33) + 5


# ---- 5. capacities
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("mode", MODES)
def test_capacities(torch_cuda, monkeypatch, novel_case, tile, mode):
    torch = torch_cuda
    _tile(monkeypatch, tile)
    m, text, off, rec, sel, want = novel_case
    ids, starts, lens, first = want[mode]
    n = ids.size
    plan = m.plan(0)
    cap = want["cap"]                                                        # the batch scan's rule: all matches of the buffer
    # exact capacities
    r = _scan(torch, plan, text, off, mode, cap, n)
    assert r.count == sel.size
    _assert_stream(r, want[mode], text.size, mode)
    # the token room one short: the need, nothing outside the room, tok_first complete and valid
    r = _scan(torch, plan, text, off, mode, cap, n - 1)
    assert (r.count, r.n_tokens) == (sel.size, n)
    assert r.ids.canaries_intact() and r.start.canaries_intact() and r.length.canaries_intact() and r.first.canaries_intact()
    assert np.array_equal(r.first.host(first.size), first)
    # the record room one short: a room that suffices, no token, the outputs untouched
    r = _scan(torch, plan, text, off, mode, cap - 1, n)
    assert r.count == cap and r.n_tokens == 0
    assert r.ids.untouched() and r.start.untouched() and r.length.untouched() and r.first.untouched()
    r1 = _scan(torch, plan, text, None, mode, cap - 1, n)                    # the same as one text: the scan's own count
    assert r1.count == cap and r1.n_tokens == 0 and r1.ids.untouched()
    # a count-only call: the count and tok_first, no token array at all
    r = _scan(torch, plan, text, off, mode, cap, 0, count_only=True)
    assert (r.count, r.n_tokens) == (sel.size, n) and np.array_equal(r.first.host(first.size), first) and r.first.canaries_intact()
    assert r.ids.untouched() and r.start.untouched() and r.length.untouched()
    plan.status()
    L = acm.lib()
    assert L.acm_gpu_tokens_tmp_bytes(plan.h, 1 << 31, 64) == 0 and L.acm_gpu_scan_tokens_tmp_bytes(plan.h, 1 << 31, 64, 1) == 0


# ---- 6. hand-made selections that break the contract
def _raw(torch, plan, text, rec, off, mode, tok_of=None, nk=0, tok_cap=4096):
    """acm_gpu_tokens_records_device itself: a _Result with rc and n_tokens"""
    L = acm.lib()
    a = np.zeros(max(rec.size, 1), po.RECORD_DTYPE)
    a[:rec.size] = rec
    d_rec = torch.from_numpy(a.view(np.int64).reshape(-1, 2).copy()).cuda()
    d_text = _dev(torch, text)
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda() if off is not None else None
    r = _outputs(torch, tok_cap, len(off) if off is not None else 0)
    d_of = torch.from_numpy(np.asarray(tok_of, np.uint32).view(np.int32).copy()).cuda() if tok_of is not None else None
    tb = L.acm_gpu_tokens_tmp_bytes(plan.h, rec.size, len(text))
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    r.rc = L.acm_gpu_tokens_records_device(plan.h, d_text.data_ptr(), len(text), 0, d_rec.data_ptr(), rec.size, None,
                                           d_off.data_ptr() if d_off is not None else None, len(off) - 1 if off is not None else 0,
                                           d_of.data_ptr() if d_of is not None else None, nk, GB, mode, r.ids.view.data_ptr(), r.start.view.data_ptr(),
                                           r.length.view.data_ptr(), tok_cap, r.res.data_ptr() + 8, r.first.view.data_ptr() if r.first is not None else None,
                                           tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    r.n_tokens = int(r.res.cpu()[1])
    return r


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("what", ["overlap", "order", "past the text", "crosses a text", "keyword id", "offsets decrease", "offsets end early"])
def test_hand_made_selections_that_break_the_contract(torch_cuda, monkeypatch, what, tile):
    torch = torch_cuda
    _tile(monkeypatch, tile)
    m, o = build_pair([b"ab", b"abcdefgh", b"x"], 1)
    text = b"abcdefghijklmnopqrstuvwxyz" * 100
    good = np.array([(5, 2, 0), (40, 8, 1), (41, 1, 2), (2599, 3, 0)], po.RECORD_DTYPE)
    good_off = [0, 1000, 1000, 2600]
    tok_of = [11, 12, 13]
    bad, off = good.copy(), list(good_off)
    if what == "overlap":
        bad[2] = (40, 1, 2)
    elif what == "order":
        bad[1], bad[2] = good[2], good[1]
    elif what == "past the text":
        bad[3] = (2600, 3, 0)
    elif what == "crosses a text":
        bad[3] = (1001, 4, 0)                                                # symbols 998 .. 1001, the boundary is at 1000
    elif what == "keyword id":
        bad[1] = (40, 8, 3)
    elif what == "offsets decrease":
        off = [0, 1000, 900, 2600]
    else:
        off = [0, 1000, 1000, 2599]
    for mode in (RUN, SYMBOL):
        # the good selection first, on a plan of its own: the call works, the flag stays down
        plan = m.plan(0)
        want = tokens_by_definition(text, good, mode, GB, tok_of, good_off)
        r = _raw(torch, plan, text, good, good_off, mode, tok_of, 3)
        assert r.rc == 0
        _assert_stream(r, want, len(text), mode)
        plan.status()
        plan = m.plan(0)                                                     # (the error flag is sticky)
        r = _raw(torch, plan, text, bad, off, mode, tok_of, 3)
        assert (r.rc, r.n_tokens) == (0, 0)
        assert r.ids.untouched() and r.start.untouched() and r.length.untouched() and r.first.untouched()
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL
    if what in ("overlap", "order", "past the text"):                        # one text, no table: the tiling is checked all the same
        plan = m.plan(0)
        r = _raw(torch, plan, text, bad, None, DROP)
        assert (r.rc, r.n_tokens) == (0, 0) and r.ids.untouched()
        with pytest.raises(acm.ACMError):
            plan.status()


# ---- 7. the host entry, the call on the machine, the padded tensor
@pytest.mark.parametrize("mode", MODES)
def test_host_entries_and_padded(torch_cuda, novel_case, mode):
    torch = torch_cuda
    m, text, off, rec, sel, want = novel_case
    ids, starts, lens, first = want[mode]
    plan = m.plan(0)
    name = {SYMBOL: "symbol", RUN: "run", DROP: "drop"}[mode]

    def same(tok):
        assert tok.n_tokens == ids.size and tok.count == sel.size
        assert np.array_equal(tok.ids, ids) and np.array_equal(tok.start, starts) and np.array_equal(tok.length, lens)
        assert np.array_equal(tok.first, first)
    same(plan.scan_tokens_host(text, off, mode=name, gap_base=GB))
    with pytest.raises(acm.ACMError) as e:                                   # ACM_GPU_E_OVERFLOW means only: the token room is too small
        plan.scan_tokens_host(text, off, mode=name, gap_base=GB, token_capacity=ids.size - 1)
    assert e.value.code == E_OVERFLOW
    texts = [text[int(off[t]):int(off[t + 1])] for t in range(off.size - 1)]
    tok = m.tokenize(texts, mode=name, gap_base=GB)
    assert m.scan_path == PATH_GPU
    same(tok)
    one = m.tokenize(text, mode=name, gap_base=GB)                           # one text: no row pointers
    rec1, sel1 = selection_of(build_pair(KEYWORDS, 1)[1], text)
    w1 = tokens_by_definition(text, sel1, mode, GB)
    assert one.first is None and np.array_equal(one.ids, w1[0]) and np.array_equal(one.start, w1[1]) and np.array_equal(one.length, w1[2])
    # the ragged rows as one tensor, against a numpy padding
    d = plan.scan_tokens(_dev(torch, text), torch.from_numpy(off.astype(np.int64)).cuda(), mode=name, gap_base=GB, capacity=want["cap"])
    assert (d.count, d.n_tokens) == (sel.size, ids.size) and d.ids.is_cuda
    lens_t = np.diff(first.astype(np.int64))
    pad = np.full((lens_t.size, int(lens_t.max())), 77, np.int64)
    for t in range(lens_t.size):
        pad[t, :lens_t[t]] = ids[int(first[t]):int(first[t + 1])]
    got = d.padded(77)
    assert got.is_cuda and tuple(got.shape) == pad.shape and np.array_equal(got.cpu().numpy(), pad)
    assert np.array_equal(tok.padded(77).cpu().numpy(), pad)                 # from the host call's numpy arrays too
    # the records-only device call on the selection the scan left
    t2 = plan.tokens_records(_dev(torch, text), d.records, d.count, torch.from_numpy(off.astype(np.int64)).cuda(), mode=name, gap_base=GB)
    assert t2.n_tokens == ids.size and np.array_equal(t2.ids[:ids.size].cpu().numpy().view(np.uint32), ids)
    assert np.array_equal(t2.first.cpu().numpy().view(np.uint64), first)
    plan.status()
