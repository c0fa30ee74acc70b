"""Search-and-replace on the GPU (acm_gpu_replace_*, acm_gpu_scan_replace_*, acm_replace;
csrc/dev_replace.h).  The expected output is always the definition of REPLACE in plain Python over
select_cases.greedy of the ORACLE's records (tests/replace_cases.py), never the library's own scan or
selection; every workload case first shows from the oracle alone that a record is selected, a record
is left out and the output differs from the input."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, TEXTS, offsets_of, oracle_batch
from tests.cases import build_pair
from tests.replace_cases import oracle_case, random_table, replace_by_definition
from tests.select_cases import greedy, oracle_records
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, kind

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
LETTERS = [bytes([c]) for c in range(97, 123)]
CANARY, GUARD = 0xA5, 64
TILES = ["256", None]                                    # ACM_GPU_REPLACE_TILE: the smallest, and the default


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _tile(monkeypatch, tile):
    monkeypatch.delenv("ACM_GPU_REPLACE_TILE", raising=False)
    if tile is not None:
        monkeypatch.setenv("ACM_GPU_REPLACE_TILE", tile)


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
    """an output buffer of n bytes, `at` bytes behind a 16-byte boundary, with canaries in front and behind"""

    def __init__(self, torch, n, at=0):
        self.whole = torch.full((GUARD + at + n + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.whole[GUARD + at:GUARD + at + n]
        self.lo, self.n = GUARD + at, n
        assert self.view.data_ptr() % 16 == at % 16

    def canaries_intact(self):
        w = self.whole.cpu().numpy()
        return bool(np.all(w[:self.lo] == CANARY) and np.all(w[self.lo + self.n:] == CANARY))

    def untouched(self):
        return bool(np.all(self.whole.cpu().numpy() == CANARY))

    def host(self, n_bytes):
        return self.whole.cpu().numpy()[self.lo:self.lo + n_bytes].copy()


def _rec_dev(torch, rec, room=None):
    a = np.zeros(max(rec.size if room is None else room, 1), po.RECORD_DTYPE)
    a[:rec.size] = rec
    return torch.from_numpy(a.view(np.int64).reshape(-1, 2).copy()).cuda()


def _rec_host(t, n):
    return np.frombuffer(t[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()


def _check(torch, plan, text, rec, sel, want, starts, replacements=None, fill=None, text_at=0, out_at=0, pos_base=0):
    """acm_gpu_scan_replace_device with exactly the room the records and the output need"""
    sb = want.dtype.itemsize
    out = _Out(torch, want.size * sb, out_at)
    r = plan.scan_replace(_dev(torch, text, text_at), replacements, fill, n_symbols=_bytes_of(text).size // sb, pos_base=pos_base,
                          capacity=rec.size, out=out.view, out_capacity=want.size, out_start=True)
    assert (r.count, r.out_symbols) == (sel.size, want.size), (r.count, sel.size, r.out_symbols, want.size)
    got = out.host(want.size * sb).view(want.dtype)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert out.canaries_intact()
    shifted = sel.copy()
    shifted["end_pos"] += np.uint64(pos_base)
    assert np.array_equal(_rec_host(r.records, r.count), shifted)
    assert np.array_equal(r.out_start[:r.count].cpu().numpy(), starts)
    plan.status()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("rlen", [0, 1, 7])
def test_entry_offsets_shrinking_and_growing(torch_cuda, monkeypatch, tile, rlen):
    """{aa, aaa} on a x 1000: 333 records of length 3 are selected; with replacements of 0, 1 and 7 symbols
    the output shrinks to 1, to 334, and grows to 2,332 symbols"""
    _tile(monkeypatch, tile)
    text = b"a" * 1000
    m, o = build_pair([b"aa", b"aaa"], 1)
    table = [b"XY", b"0123456"[:rlen]]
    rec, sel, want, starts = oracle_case(o, text, table)
    assert sel.size == 333 and want.size == 1 + 333 * rlen
    _check(torch_cuda, m.plan(0), text, rec, sel, want, starts, table)


def _planted(rng, n, word, every):
    text = rng.integers(97, 123, size=n, dtype=np.uint8)
    for at in range(17, n - len(word), every):
        text[at:at + len(word)] = np.frombuffer(word, np.uint8)
    return text


@pytest.mark.parametrize("tile", TILES)
def test_all_16_misalignments(torch_cuda, monkeypatch, tile):
    """a keyword every 301 symbols whose replacement is one symbol longer: (source - destination) mod 16
    goes through every residue along the text; the buffers begin 0, 1, 3 and 8 bytes behind a 16-byte
    boundary"""
    _tile(monkeypatch, tile)
    text = _planted(np.random.default_rng(16), 70000, b"needle", 301)
    m, o = build_pair([b"needle", b"dle"], 1)
    table = [b"NEEDLES", b"DLE!"]
    rec, sel, want, starts = oracle_case(o, text, table)
    assert sel.size >= 230
    residues = set(int((starts[j] + len(table[int(sel[j]["keyword_id"])]) - (int(sel[j]["end_pos"]) + 1)) % 16) for j in range(sel.size))
    assert residues == set(range(16))                     # of the stretch behind every replacement
    plan = m.plan(0)
    for text_at in (0, 1, 3, 8):
        for out_at in (0, 1, 3, 8):
            _check(torch_cuda, plan, text, rec, sel, want, starts, table, text_at=text_at, out_at=out_at)


@pytest.mark.parametrize("tile", TILES)
def test_dense_every_symbol_is_a_match(torch_cuda, monkeypatch, tile):
    _tile(monkeypatch, tile)
    rng = np.random.default_rng(26)
    text = rng.integers(97, 123, size=70000, dtype=np.uint8)
    keywords = LETTERS + [b"ab"]                          # (`ab` leaves its `a` and its `b` out)
    m, o = build_pair(keywords, 1)
    table = random_table(rng, len(keywords), 0, 3)
    rec, sel, want, starts = oracle_case(o, text, table)
    assert int(sel["length"].sum()) == text.size          # the selection covers the text
    plan = m.plan(0)
    _check(torch_cuda, plan, text, rec, sel, want, starts, table, out_at=3)
    rec, sel, want, starts = oracle_case(o, text, fill=ord("#"))
    assert want.size == text.size and np.all(want == ord("#"))
    _check(torch_cuda, plan, text, rec, sel, want, starts, fill=ord("#"), out_at=1)


@pytest.mark.parametrize("where", ["front", "back", "adjacent"])
def test_long_replacement_tiles_inside_it(torch_cuda, monkeypatch, where):
    """one symbol becomes 5,000: tiles of 256 bytes lie wholly inside one replacement"""
    _tile(monkeypatch, "256")
    rng = np.random.default_rng(5000)
    text = rng.integers(97, 120, size=3000, dtype=np.uint8)       # a-w: no x
    text[1500:1503] = np.frombuffer(b"she", np.uint8)
    if where == "front":
        text[0] = ord("x")
    elif where == "back":
        text[-1] = ord("x")
    else:
        text[700:702] = ord("x")
    m, o = build_pair([b"x", b"he", b"she"], 1)
    table = [rng.integers(48, 58, size=5000, dtype=np.uint8), b"", b"S"]
    rec, sel, want, starts = oracle_case(o, text, table)
    assert np.count_nonzero(sel["keyword_id"] == 0) == (2 if where == "adjacent" else 1)
    _check(torch_cuda, m.plan(0), text, rec, sel, want, starts, table, out_at=8)
    rec, sel, want, starts = oracle_case(o, text, fill=ord("_"))
    _check(torch_cuda, m.plan(0), text, rec, sel, want, starts, fill=ord("_"))


@pytest.mark.parametrize("tile", TILES)
def test_long_gap_tiles_without_a_record(torch_cuda, monkeypatch, tile):
    _tile(monkeypatch, tile)
    text = b"she" + b"q" * 50000 + b"she" + b"qq"
    m, o = build_pair([b"she", b"he"], 1)
    table = [b"[woman]", b"[man]"]
    rec, sel, want, starts = oracle_case(o, text, table)
    assert sel.size == 2 and int(sel[1]["end_pos"]) - int(sel[0]["end_pos"]) == 50003
    _check(torch_cuda, m.plan(0), text, rec, sel, want, starts, table, text_at=3, out_at=1)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("sym_size", [1, 2, 4, 8])
def test_symbol_sizes(torch_cuda, monkeypatch, tile, sym_size):
    _tile(monkeypatch, tile)
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[sym_size]
    rng = np.random.default_rng(80 + sym_size)
    alphabet = (np.arange(1, 5, dtype=np.uint64) * np.uint64(0x0102030405060708 & ((1 << (8 * sym_size)) - 1))).astype(dtype)
    assert np.unique(alphabet).size == 4
    keywords = [alphabet[[0, 1]], alphabet[[0, 1, 2]], alphabet[[1]], alphabet[[3, 3, 0]], alphabet[[2, 2]]]
    text = alphabet[rng.integers(0, 4, size=20011)]
    m, o = build_pair(keywords, sym_size)
    other = (np.arange(9, 31, dtype=np.uint64) * np.uint64(0x0807060504030201 & ((1 << (8 * sym_size)) - 1))).astype(dtype)
    table = [other[rng.integers(0, other.size, size=k)] for k in (3, 0, 1, 5, 2)]
    rec, sel, want, starts = oracle_case(o, text, table)
    plan = m.plan(0)
    for at in (0, sym_size):
        _check(torch_cuda, plan, text, rec, sel, want, starts, table, text_at=at, out_at=(3 * sym_size) % 16)
    rec, sel, want, starts = oracle_case(o, text, fill=other[7])
    _check(torch_cuda, plan, text, rec, sel, want, starts, fill=other[7], out_at=sym_size)


def _overlap_across_the_delta(text):
    """a keyword of the plan's own tables (the first 300 of 450) written into a copy of the text with a
    keyword of the delta (300 .. 448) beginning on its last symbol: one record of each overlap, and
    the selection drops the delta's (tests/test_select_gpu.py has the same case)"""
    kd, ko = acm.synth.keywords(450)
    a, b = next((a, b) for a in range(300) for b in range(300, 449) if kd[ko[a + 1] - 1] == kd[ko[b]] and ko[b + 1] - ko[b] > 1)
    both = np.concatenate([kd[ko[a]:ko[a + 1]], kd[ko[b] + 1:ko[b + 1]]])
    text = text.copy()
    text[50_000:50_000 + both.size] = both
    return text


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind(torch_cuda, monkeypatch, kat, novel_bytes, name):
    torch = torch_cuda
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    text = text[:1 << 17]
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    if name == "csr":
        text = text[1:]
    if name == "delta":
        text = _overlap_across_the_delta(text)
    rng = np.random.default_rng(len(name))
    lo, hi = (1 << 40, 1 << 41) if text.dtype.itemsize == 8 else (200, 250) if text.dtype.itemsize == 1 else (60000, 60100)
    table = random_table(rng, o.nb_keywords, 0, 5, (lo, hi), text.dtype)
    rec, sel, want, starts = oracle_case(o, text, table)
    if name == "classes":                                 # the stretches keep the text's own case: Mrs / mrs / MRS are one class
        lower = np.frombuffer(bytes(text).lower(), np.uint8)
        assert not np.array_equal(lower, text)
        wrong, _ = replace_by_definition(lower, sel, table)
        assert wrong.size == want.size and not np.array_equal(wrong, want)
    if name == "delta":
        assert plan.tally_keywords == o.nb_keywords == 450 and int(sel["keyword_id"].max()) >= 300
    _check(torch, plan, text, rec, sel, want, starts, table, text_at=1 if name == "csr" else 0, out_at=text.dtype.itemsize)
    if name == "delta":                                   # a table without the delta's keywords
        with pytest.raises(acm.ACMError) as e:
            plan.scan_replace(_dev(torch, text), table[:300], capacity=rec.size)
        assert e.value.code == E_ARG
        with pytest.raises(acm.ACMError) as e:
            plan.scan_replace_host(text, table[:449])
        assert e.value.code == E_ARG
    got, n = m.replace(text, table)
    assert n == sel.size and np.array_equal(got, want)
    assert m.scan_path == (PATH_CLASSES if name == "classes" else PATH_GPU)
    got, n = m.replace(text, fill=table[0][:1] if table[0].size else lo)
    assert n == sel.size and got.size == text.size


def test_nonzero_pos_base(torch_cuda):
    text = b"To ushers: he found his pencil, but she could not find hers." * 20
    m, o = build_pair([b"he", b"she", b"his", b"hers"], 1)
    table = [b"", b"SHE!", b"hi", b"[theirs]"]
    rec, sel, want, starts = oracle_case(o, text, table)
    _check(torch_cuda, m.plan(0), text, rec, sel, want, starts, table, pos_base=(1 << 33) + 5, out_at=1)


def _raw(torch, plan, text, rec, data, off, nk, out, out_capacity, pos_base=0, n=None, count=None):
    """acm_gpu_replace_records_device itself: (rc, *d_out_symbols)"""
    L = acm.lib()
    d_text, d_rec = _dev(torch, text), _rec_dev(torch, rec)
    d_data = _dev(torch, data)
    d_off = torch.from_numpy(np.asarray(off, np.int64)).cuda() if off is not None else None
    n = rec.size if n is None else n
    res = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_replace_tmp_bytes(plan.h, n, len(text))
    assert tb > 0
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_replace_records_device(plan.h, d_text.data_ptr(), len(text), pos_base, d_rec.data_ptr(), n,
                                          count.data_ptr() if count is not None else None, d_data.data_ptr(),
                                          d_off.data_ptr() if d_off is not None else None, nk, out.view.data_ptr(), out_capacity, res.data_ptr(),
                                          None, tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    return rc, int(res.item())


@pytest.mark.parametrize("what", ["overlap", "order", "past the text", "in front of the text", "keyword id", "repl_off"])
def test_hand_made_selections_that_break_the_contract(torch_cuda, what):
    torch = torch_cuda
    m, o = build_pair([b"ab", b"abcdefgh", b"x"], 1)
    text = b"abcdefghijklmnopqrstuvwxyz" * 100
    good = np.array([(5, 2, 0), (40, 8, 1), (41, 1, 2), (2599, 3, 0)], po.RECORD_DTYPE)
    data, off, nk = b"0123456789", [0, 2, 7, 10], 3
    bad = good.copy()
    if what == "overlap":
        bad[2] = (40, 1, 2)
    elif what == "order":
        bad[1], bad[2] = good[2], good[1]
    elif what == "past the text":
        bad[3] = (2600, 3, 0)
    elif what == "in front of the text":
        bad[0] = (1, 3, 0)
    elif what == "keyword id":
        bad[1] = (40, 8, 3)
    else:
        off = [0, 7, 2, 10]
    # the good selection first, on a plan of its own: the call works, the flag stays down
    plan = m.plan(0)
    want, _ = replace_by_definition(text, good, [b"01", b"23456", b"789"])
    out = _Out(torch, want.size)
    rc, n_out = _raw(torch, plan, text, good, data, [0, 2, 7, 10], 3, out, want.size)
    assert (rc, n_out) == (0, want.size) and np.array_equal(out.host(want.size), want) and out.canaries_intact()
    plan.status()
    plan = m.plan(0)                                      # (the error flag is sticky)
    out = _Out(torch, want.size + 64)
    rc, n_out = _raw(torch, plan, text, bad, data, off, nk, out, want.size + 64)
    assert (rc, n_out) == (0, 0) and out.untouched()
    with pytest.raises(acm.ACMError) as e:
        plan.status()
    assert e.value.code == E_INTERNAL
    if what not in ("keyword id", "repl_off"):            # mask mode checks the tiling too
        plan = m.plan(0)
        rc, n_out = _raw(torch, plan, text, bad, b"*", None, 0, out, want.size + 64)
        assert (rc, n_out) == (0, 0) and out.untouched()
        with pytest.raises(acm.ACMError):
            plan.status()


def test_replace_of_a_batch_is_the_concatenation_of_the_texts(torch_cuda):
    torch = torch_cuda
    m, o = build_pair(KEYWORDS, 1)
    texts = TEXTS * 30
    off = offsets_of(texts)
    table = [b"HE", b"", b"theirs", b"$"]
    all_rec, _, first = oracle_batch(o, texts)
    per_text = [replace_by_definition(t, greedy(oracle_records(o, t)), table)[0] for t in texts]
    want = np.concatenate(per_text)
    sel_all = np.concatenate([greedy(all_rec[int(first[t]):int(first[t + 1])]) for t in range(len(texts))])
    assert 0 < sel_all.size < all_rec.size and want.size != int(off[-1])
    plan = m.plan(0)
    whole = b"".join(texts)
    d_text = _dev(torch, whole)
    rec, _, _ = plan.scan_batch(d_text, torch.from_numpy(off.astype(np.int64)).cuda())
    assert np.array_equal(rec, all_rec)
    sel, n = plan.select_records(_rec_dev(torch, rec), rec.size, 0, int(off[-1]))
    assert n == sel_all.size
    out = _Out(torch, want.size, 3)
    r = plan.replace_records(d_text, sel, n, table, out=out.view, out_capacity=want.size)
    assert r.out_symbols == want.size and np.array_equal(out.host(want.size), want) and out.canaries_intact()
    plan.status()


def test_overflows(torch_cuda):
    torch = torch_cuda
    m, o = build_pair(KEYWORDS, 1)
    text = b"".join(TEXTS) * 50
    table = [b"HE", b"", b"theirs", b"$$"]
    rec, sel, want, starts = oracle_case(o, text, table)
    plan = m.plan(0)
    d_text = _dev(torch, text)
    # the output one symbol short: the exact need, nothing outside the room, the repeat succeeds
    out = _Out(torch, want.size - 1, 1)
    r = plan.scan_replace(d_text, table, capacity=rec.size, out=out.view, out_capacity=want.size - 1)
    assert (r.count, r.out_symbols) == (sel.size, want.size) and out.canaries_intact()
    _check(torch, plan, text, rec, sel, want, starts, table, out_at=1)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_replace_host(np.frombuffer(text, np.uint8), table, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW
    # the records one short: the scan's count, no output
    out = _Out(torch, want.size)
    r = plan.scan_replace(d_text, table, capacity=rec.size - 1, out=out.view, out_capacity=want.size)
    assert (r.count, r.out_symbols) == (rec.size, 0) and out.untouched()
    # arguments
    L = acm.lib()
    assert L.acm_gpu_replace_tmp_bytes(plan.h, 1 << 31, 64) == 0 and L.acm_gpu_scan_replace_tmp_bytes(plan.h, 1 << 31, 64) == 0
    with pytest.raises(acm.ACMError) as e:                # the output inside the text
        plan.scan_replace(d_text, fill=b"*", capacity=rec.size, out=d_text[16:], out_capacity=16)
    assert e.value.code == E_ARG
    plan.status()


def test_empty_text_and_text_without_a_match(torch_cuda):
    torch = torch_cuda
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    table = [b"HE", b"", b"theirs", b"$$"]
    quiet = b"q" * 3001
    for kw in ({"replacements": table}, {"fill": b"*"}):
        out = _Out(torch, 3001, 1)
        r = plan.scan_replace(_dev(torch, quiet, 3), capacity=16, out=out.view, out_capacity=3001, **kw)
        assert (r.count, r.out_symbols) == (0, 3001) and bytes(out.host(3001)) == quiet and out.canaries_intact()
        out = _Out(torch, 16)
        r = plan.scan_replace(_dev(torch, b"0123456789abcdef")[:0], capacity=16, out=out.view, out_capacity=16, **kw)
        assert (r.count, r.out_symbols) == (0, 0) and out.untouched()
        got, n = plan.scan_replace_host(np.frombuffer(quiet, np.uint8), **kw)
        assert n == 0 and bytes(got) == quiet
        got, n = plan.scan_replace_host(np.zeros(0, np.uint8), **kw)
        assert n == 0 and got.size == 0
        got, n = m.replace(quiet, **kw)
        assert n == 0 and bytes(got) == quiet
        got, n = m.replace(b"", **kw)
        assert n == 0 and got.size == 0
    plan.status()


@pytest.mark.parametrize("path", [PATH_GPU, PATH_CLASSES])
def test_more_than_2_mi_matches_and_no_record_capacity(torch_cuda, kat, path):
    """{a, b, ab} on 3 MiB over a, b, c: 2.4 M matches, more than the 2 Mi records any default room in this
    library holds; the host entries count first and size the record room themselves.  The text is 64
    copies of a block that ends with `c`, which no keyword holds: no match crosses a block, so the
    expectation is the block's (by the definition over the oracle's records), 64 times -- shown on two
    blocks from the oracle before it is used."""
    rng = np.random.default_rng(2)
    letters = np.frombuffer(b"abcABC" if path == PATH_CLASSES else b"abc", np.uint8)
    block = letters[rng.integers(0, letters.size, size=49152)].copy()
    block[-1] = ord("c")
    keywords = [b"a", b"b", b"ab"]
    if path == PATH_CLASSES:
        cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
        m, o = acm.Machine(1, cmp=cmp), po.Oracle(1, po.MEYER85, cmp=cmp)
        for kw in keywords:
            m.add_keyword(kw)
            o.add_keyword(kw)
        m.set_symbol_bytes(1)
    else:
        m, o = build_pair(keywords, 1)
    table = [b"<1>", b"", b"two"]
    rec, sel, want, _ = oracle_case(o, block, table)
    two = oracle_records(o, np.concatenate([block, block]))
    shifted = rec.copy()
    shifted["end_pos"] += np.uint64(block.size)
    assert np.array_equal(two, np.concatenate([rec, shifted]))
    copies = 64
    assert rec.size * copies > 2 << 20
    text, want = np.tile(block, copies), np.tile(want, copies)
    got, n = m.replace(text, table)
    assert m.scan_path == path
    assert n == sel.size * copies and got.size == want.size and np.array_equal(got, want)
    plan = m.plan_classes(0) if path == PATH_CLASSES else m.plan(0)
    got, n = plan.scan_replace_host(text, table)
    assert n == sel.size * copies and np.array_equal(got, want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_replace_host(text, table, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW
    mwant = np.tile(replace_by_definition(block, sel, fill=ord("*"))[0], copies)
    got, n = plan.scan_replace_host(text, fill=b"*")
    assert n == sel.size * copies and np.array_equal(got, mwant)
    plan.status()
