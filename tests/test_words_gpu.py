"""Whole-word matches on the GPU (acm_gpu_words_*, acm_gpu_scan_words_*, acm_scan_words;
csrc/dev_words.h).  The expected answer is always the definition of WORDS in plain Python over the
ORACLE's records or over hand-made records (tests/words_cases.py), never the library's own scan or
filter.  Texts are a few KiB and hold a few thousand records; one case has more records than the
capped grid has blocks of 64, so that blocks stride over tiles."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import broken_last_pair, offsets_of, oracle_batch
from tests.cases import build_pair
from tests.replace_cases import replace_by_definition
from tests.select_cases import greedy
from tests.tally_cases import PATH_CLASSES, PATH_GPU, kind
from tests.words_cases import ASCII_WORD, BOTH, LEFT, RIGHT, as_set, novel_case, oracle_records, words, words_by_re

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
KEYWORDS = [b"he", b"she", b"his", b"hers", b"the", b"e.g.", b"New York", b"x"]
TEXT = b"the she he, her hers_he e.g. New York's New York x xx ax x_ _x (x) ushers e.g.x his"
SIXTEEN = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F)] + [(c, c + 1) for c in range(0x61, 0x7B, 2) if c != 0x73] + [(0x73, 0x74)]
PATTERN = 0x0123456789ABCDEF


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


def _rec_dev(torch, rec, room=None, fill=None):
    a = np.zeros(max(rec.size if room is None else room, 1), po.RECORD_DTYPE)
    if fill is not None:
        a["end_pos"] = fill
    a[:rec.size] = rec
    return torch.from_numpy(a.view(np.int64).reshape(-1, 2).copy()).cuda()


def _rec_host(t, n):
    return np.frombuffer(t[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()


def _same(got, want, what=None):
    assert got.size == want.size and np.array_equal(got.astype(po.RECORD_DTYPE), want), (what, got.size, want.size, got[:8], want[:8])


def _sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(DTYPE[sb])


def _ranges(ranges, sb):
    return [(lo | HIGH[sb], hi | HIGH[sb]) for lo, hi in ranges]


def _filter(plan, dev, rec, **kw):
    """Plan.words_records on the records `rec` (host): the kept records (host)"""
    torch = __import__("torch")
    out, cnt = plan.words_records(dev, _rec_dev(torch, rec), rec.size, **kw)
    n = int(cnt.item())
    assert n <= rec.size
    return _rec_host(out, n)


def _hand_made(positions, length=1, keyword=0):
    rec = np.zeros(len(positions), po.RECORD_DTYPE)
    rec["end_pos"] = np.asarray(positions, np.uint64) + np.uint64(length - 1)
    rec["length"] = length
    rec["keyword_id"] = keyword
    return rec


_plans = {}


def _plan(sb, monkeypatch, kat):
    """a plan of the symbol size, made once: the dense, the start-parallel and the interned 8-byte kind of
    tests/tally_cases.py; no kind has 2-byte symbols, so a small dictionary of our own there.  The filter
    uses a plan for its device, its symbol size and its grid cap only."""
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


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_edges_of_the_buffer_and_every_alignment(torch_cuda, monkeypatch, kat, sb):
    """a match at symbol 0 and one that ends at n - 1; the symbols in front of the buffer and behind it are
    word symbols and must not be looked at -- with d_text at an aligned allocation and one symbol past it.
    The same plans filter the crafted text under all three flags and under 16 ranges."""
    plan = _plan(sb, monkeypatch, kat)
    text = b"he said: she"
    rec = oracle_records(KEYWORDS, text)
    want = words(rec, text)
    assert as_set(want) == {(1, 2, 0), (11, 3, 1)} and rec.size == 3
    sym = _sym(text, sb)
    word = _sym(b"a", sb)
    for k in (16 // sb, 1):                                                              # 16-byte aligned, and one symbol past it
        whole = _dev(torch_cuda, np.concatenate([np.repeat(word, k), sym, np.repeat(word, 16)]))
        dev = whole[k:k + sym.size]
        assert whole.data_ptr() % 16 == 0 and dev.data_ptr() % 16 == k * sb % 16 and dev.is_contiguous()
        for flags, name in ((LEFT, "left"), (RIGHT, "right"), (BOTH, "both")):
            _same(_filter(plan, dev, rec, ranges=_ranges(ASCII_WORD, sb), flags=name), words(rec, text, flags=flags), (k, name))
        # the buffer one symbol shorter: the last symbol is now outside it and is no neighbour of anything
        inner = rec[(rec["end_pos"] < sym.size - 1)]
        _same(_filter(plan, whole[k:k + sym.size - 1], inner, ranges=_ranges(ASCII_WORD, sb)), words(inner, text[:-1]), k)
    rec = oracle_records(KEYWORDS, TEXT)
    dev = _dev(torch_cuda, _sym(TEXT, sb))
    sizes = set()
    for flags, name in ((LEFT, "left"), (RIGHT, "right"), (BOTH, "both")):
        want = words(rec, TEXT, flags=flags)
        assert as_set(want) == words_by_re(KEYWORDS, TEXT, flags)
        _same(_filter(plan, dev, rec, ranges=_ranges(ASCII_WORD, sb), flags=name), want, name)
        sizes.add(want.size)
    assert len(sizes) == 3 and max(sizes) < rec.size                                    # LEFT, RIGHT and BOTH differ
    _same(_filter(plan, dev, rec, ranges=_ranges(SIXTEEN, sb)), words(rec, TEXT))
    assert words(rec, TEXT, ranges=SIXTEEN[:15]).size != words(rec, TEXT).size          # the sixteenth range counts
    _same(_filter(plan, dev, rec, ranges=_ranges(SIXTEEN[:15], sb)), words(rec, TEXT, ranges=SIXTEEN[:15]))
    if sb > 1:   # the plain ASCII ranges hold none of these symbols: everything is whole-word
        _same(_filter(plan, dev, rec), rec)
    # pos_base
    shifted = rec.copy()
    shifted["end_pos"] += 5000
    want = words(rec, TEXT).copy()
    want["end_pos"] += 5000
    _same(_filter(plan, dev, shifted, ranges=_ranges(ASCII_WORD, sb), pos_base=5000), want)
    plan.status()


def test_text_boundaries_of_a_packed_batch(torch_cuda):
    texts = [b"", b"", b"the", b"he", b"hers", b"us", b"hers x", b"", b"", b"(she) ", b"x", b"", b"he"] * 20 + [b""]
    packed = b"".join(texts)
    off = offsets_of(texts)
    m, o = build_pair(KEYWORDS, 1)
    rec = oracle_records(KEYWORDS, packed)
    want = words(rec, packed, offsets=off)
    got_set = as_set(want)
    # `he` is a whole text between "the" and "hers": kept; `she` of "us|hers" spans a cut: dropped
    assert (4, 2, 0) in got_set and (8, 4, 3) in got_set and (12, 3, 1) in as_set(rec) and (12, 3, 1) not in got_set
    per_text = set()
    for t in range(len(texts)):
        per_text |= {(e + int(off[t]), l, k) for e, l, k in words_by_re(KEYWORDS, texts[t])}
    assert got_set == per_text and 0 < want.size < rec.size
    plan = m.plan(0)
    dev, d_off = _dev(torch_cuda, packed), _dev(torch_cuda, off.astype(np.int64))
    for flags, name in ((LEFT, "left"), (RIGHT, "right"), (BOTH, "both")):
        _same(_filter(plan, dev, rec, offsets=d_off, flags=name), words(rec, packed, offsets=off, flags=flags), name)
    # the filter of acm_scan_batch's records is the same: no record of a batch scan spans a cut
    batch_rec, _, _ = plan.scan_batch(dev, d_off)
    assert np.array_equal(batch_rec, oracle_batch(o, texts)[0]) and batch_rec.size < rec.size
    _same(_filter(plan, dev, batch_rec, offsets=d_off), want)
    # the fused call with offsets, device and host
    r, c, _ = plan.scan_words(dev, offsets=d_off, capacity=rec.size)
    _same(_rec_host(r, int(c.item())), want)
    _same(plan.scan_words_host(np.frombuffer(packed, np.uint8), offsets=off), want)
    plan.status()                                                                       # a record across a cut is no error


def _pairs(seps):
    """the text "x" + seps[0] + "x" + seps[1] + ...: record i is the `x` at 2 i"""
    t = np.full(2 * len(seps), ord("x"), np.uint8)
    t[1::2] = np.frombuffer(bytes(seps), np.uint8)
    return t.tobytes(), _hand_made(np.arange(len(seps)) * 2)


@pytest.mark.parametrize("tile", [None, 64, 128])
def test_wave_and_tile_seams(torch_cuda, monkeypatch, tile):
    if tile:
        monkeypatch.setenv("ACM_GPU_WORDS_TILE", str(tile))
    m, o = build_pair([b"x"], 1)
    plan = m.plan(0)
    T = tile or 4096
    rng = np.random.default_rng(64)
    counts = sorted({0, 1, 63, 64, 65, T - 1, T, T + 1, 40 * T + 7 if tile else 2 * T + 65})
    for n in counts:
        for what in ("all", "none", "alternating", "random", "shuffled"):
            seps = {"all": b" " * n, "none": b"a" * n, "alternating": b" a" * (n // 2) + b" " * (n % 2)}.get(what)
            if seps is None:
                seps = bytes(rng.choice(np.frombuffer(b" a_.", np.uint8), size=n))
            text, rec = _pairs(seps)
            flags = RIGHT if what == "alternating" else BOTH
            if what == "shuffled":
                rec = rec[rng.permutation(rec.size)]
            want = words(rec, text, flags=flags) if n else rec
            if n > 1:
                assert want.size == {"all": n, "none": 0, "alternating": (n + 1) // 2}.get(what, want.size)
            if n == 0:
                out, cnt = plan.words_records(_dev(torch_cuda, b"q" * 16), _rec_dev(torch_cuda, rec), 0, flags=flags)
                assert int(cnt.item()) == 0
                continue
            # record for record: the kept records keep the order of the input across waves and tiles
            _same(_filter(plan, _dev(torch_cuda, text), rec, flags=flags), want, (tile, n, what))
    plan.status()


def test_more_tiles_than_the_grid_has_blocks(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles"""
    monkeypatch.setenv("ACM_GPU_WORDS_TILE", "64")
    m, o = build_pair([b"x"], 1)
    plan = m.plan(0)
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus + 3) * 64 + 65
    rng = np.random.default_rng(8)
    seps = rng.choice(np.frombuffer(b" a", np.uint8), size=n)
    text, rec = _pairs(seps.tobytes())
    # the definition for this shape, without a loop: `x` at 2 i is kept iff seps[i - 1] and seps[i] are blanks
    blank = seps == ord(" ")
    keep = blank & np.concatenate([[True], blank[:-1]])
    assert np.array_equal(words(rec[:2000], text[:4000] + b"x"), rec[:2000][keep[:2000]])   # (the loop agrees where it is affordable)
    got = _filter(plan, _dev(torch_cuda, text), rec)
    _same(got, rec[keep])
    assert 0 < got.size < n
    plan.status()


def test_counts_on_the_device_and_overflow(torch_cuda):
    torch = torch_cuda
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    text = TEXT * 13
    rec = oracle_records(KEYWORDS, text)
    want = words(rec, text)
    assert 0 < want.size < rec.size and rec.size > 256
    dev = _dev(torch, text)
    # d_n NULL: n is the count
    _same(_filter(plan, dev, rec), want)
    # d_n given: n is the room; the output count in a tensor of its own, then in d_n itself
    room = rec.size + 100
    d_rec = _rec_dev(torch, rec, room, fill=PATTERN)
    count = torch.tensor([rec.size], dtype=torch.int64, device="cuda")
    out, cnt = plan.words_records(dev, d_rec, room, count=count)
    assert cnt.data_ptr() != count.data_ptr() and int(count.item()) == rec.size
    _same(_rec_host(out, int(cnt.item())), want)
    out, cnt = plan.words_records(dev, d_rec, room, count=count, out_count=count)
    assert cnt is count
    _same(_rec_host(out, int(count.item())), want)
    # a scan that overflowed: *d_n > room -- nothing is kept, *d_count = *d_n, d_out untouched
    prefilled = _hand_made(np.full(room, PATTERN, np.uint64), 7, 7)
    for same in (False, True):
        count = torch.tensor([room + 1], dtype=torch.int64, device="cuda")
        d_out = _rec_dev(torch, prefilled)
        out, cnt = plan.words_records(dev, d_rec, room, count=count, out=d_out, out_count=count if same else None)
        assert int(cnt.item()) == room + 1 and int(count.item()) == room + 1
        assert np.array_equal(_rec_host(d_out, room), prefilled)
    # no room at all: a count that came in stays
    count = torch.tensor([12345], dtype=torch.int64, device="cuda")
    out, cnt = plan.words_records(dev, d_rec, 0, count=count)
    assert int(cnt.item()) == 12345
    plan.status()


def test_words_device_arguments(torch_cuda):
    torch = torch_cuda
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    L = acm.lib()
    rec = oracle_records(KEYWORDS, TEXT)
    dev = _dev(torch, TEXT)
    d_rec = _rec_dev(torch, rec, 2 * rec.size)
    prefilled = _hand_made(np.full(rec.size, PATTERN, np.uint64), 7, 7)
    d_out = _rec_dev(torch, prefilled)
    count = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_words_tmp_bytes(plan.h, rec.size, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    r = np.asarray(ASCII_WORD, np.uint8).reshape(-1)
    reversed_pair = np.array([0x30, 0x39, 0x7A, 0x61], np.uint8)

    def call(plan_h=plan.h, text=dev.data_ptr(), ranges=r.ctypes.data, n_ranges=4, flags=3, records=d_rec.data_ptr(), n=rec.size, out=d_out.data_ptr(),
             cnt=count.data_ptr(), scratch=tmp.data_ptr(), tmp_bytes=tb, offsets=None, n_texts=0):
        return L.acm_gpu_words_records_device(plan_h, text, len(TEXT), 0, offsets, n_texts, ranges, n_ranges, flags, records, n, None, out, cnt,
                                              scratch, tmp_bytes, None)
    assert tb > 0 and L.acm_gpu_words_tmp_bytes(plan.h, 1 << 31, 0) == 0 and L.acm_gpu_scan_words_tmp_bytes(plan.h, 1 << 31, 64, 0) == 0
    assert call(plan_h=None) == E_ARG and call(text=None) == E_ARG and call(records=None) == E_ARG and call(out=None) == E_ARG
    assert call(cnt=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(ranges=None) == E_ARG and call(n_ranges=0) == E_ARG and call(n_ranges=17) == E_ARG and call(flags=0) == E_ARG and call(flags=4) == E_ARG
    assert call(ranges=reversed_pair.ctypes.data, n_ranges=2) == E_ARG
    # d_out overlapping d_records, at either end
    assert call(out=d_rec.data_ptr()) == E_ARG and call(out=d_rec.data_ptr() + 16 * (rec.size - 1)) == E_ARG
    assert call(out=d_rec.data_ptr() - 16 * (rec.size - 1)) == E_ARG
    assert call(offsets=dev.data_ptr(), n_texts=0) == E_ARG                            # no text, but symbols
    torch.cuda.synchronize()
    assert np.array_equal(_rec_host(d_out, rec.size), prefilled) and int(count.item()) == 0x5A5A      # nothing was touched
    assert call(out=d_rec.data_ptr() + 16 * rec.size) == 0                              # right behind the records: no overlap
    torch.cuda.synchronize()
    _same(_rec_host(d_rec[rec.size:], int(count.item())), words(rec, TEXT))
    assert call() == 0
    torch.cuda.synchronize()
    _same(_rec_host(d_out, int(count.item())), words(rec, TEXT))
    plan.status()


def test_a_class_plan_tests_the_callers_own_symbols(torch_cuda, monkeypatch, kat, novel_bytes):
    """the case-folding comparator of tests/test_classes.py and the range a-z alone: an upper-case
    neighbour is no word symbol, though the plan's scan takes it for its lower-case letter"""
    m, o, _, make_plan, plan_ok, _ = kind("classes", monkeypatch, kat)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    text = b"THE he SHE she hErs hersX Xhers xhers MRS mrs. " + novel_bytes[:3000]
    rec = o.scan(text)
    lower = [(0x61, 0x7A)]
    want = words(rec, text, ranges=lower)
    ascii_want = words(rec, text)
    # `HE` of "THE" (keyword He): its neighbour is `T`
    assert (2, 2, 0) in as_set(want) and (2, 2, 0) not in as_set(ascii_want) and 0 < ascii_want.size < want.size < rec.size
    dev = _dev(torch_cuda, text)
    _same(_filter(plan, dev, rec, ranges=lower), want)
    _same(_filter(plan, dev, rec), ascii_want)
    r, c, _ = plan.scan_words(dev, ranges=lower, capacity=rec.size)
    _same(_rec_host(r, int(c.item())), want)
    _same(m.scan_words(text, ranges=lower), want)
    assert m.scan_path == PATH_CLASSES
    plan.status()


def fused_calls_on_plan(torch_cuda, plan, sb, text, rec, want):
    """the fused calls and the filter behind both scans, through every call that takes a plan (of novel_case ()'s keywords
    as symbols of sb bytes, however it came to hold them: tests/test_growth_gpu.py calls this with grown plans); returns
    (symbols, ranges)"""
    sym = _sym(text, sb)
    dev = _dev(torch_cuda, sym)
    ranges = _ranges(ASCII_WORD, sb)
    # scan_words is the filter of scan_ordered
    all_rec, all_cnt, _ = plan.scan_ordered(dev, capacity=rec.size)
    assert int(all_cnt.item()) == rec.size
    assert np.array_equal(_rec_host(all_rec, rec.size), rec)
    for flags, name in ((LEFT, "left"), (RIGHT, "right"), (BOTH, "both")):
        r, c, _ = plan.scan_words(dev, ranges=ranges, flags=name, capacity=rec.size)
        _same(_rec_host(r, int(c.item())), words(rec, text, flags=flags), (sb, name))
        out, cnt = plan.words_records(dev, all_rec, rec.size, ranges=ranges, flags=name, count=all_cnt)
        _same(_rec_host(out, int(cnt.item())), words(rec, text, flags=flags), (sb, name))
    # the filter of the UNORDERED scan keeps the same set
    raw, raw_cnt = plan.scan(dev, capacity=rec.size)
    out, cnt = plan.words_records(dev, raw, rec.size, ranges=ranges, count=raw_cnt)
    assert as_set(_rec_host(out, int(cnt.item()))) == as_set(want) and int(cnt.item()) == want.size
    # capacity too small for ALL matches: the scan's count
    r, c, _ = plan.scan_words(dev, ranges=ranges, capacity=rec.size - 1)
    assert int(c.item()) == rec.size
    r, c, _ = plan.scan_words(dev, ranges=ranges, capacity=want.size)
    assert int(c.item()) == rec.size
    # host memory in, blocking: an overflow reports a capacity that suffices
    with pytest.raises(acm.ACMError) as e:
        plan.scan_words_host(sym, ranges=ranges, capacity=rec.size - 1)
    assert e.value.code == E_OVERFLOW
    n = C.c_uint64(0)
    small = np.zeros(rec.size - 1, po.RECORD_DTYPE)
    rr = np.asarray(ranges, np.uint64).astype(DTYPE[sb]).reshape(-1)
    assert acm.lib().acm_gpu_scan_words_host(plan.h, sym.ctypes.data, sym.size, 0, None, 0, rr.ctypes.data, 4, 3, small.ctypes.data, small.size,
                                             C.byref(n)) == E_OVERFLOW and n.value == rec.size
    _same(plan.scan_words_host(sym, ranges=ranges, capacity=int(n.value)), want)
    _same(plan.scan_words_host(sym, ranges=ranges), want)
    # an empty text and a text without a match
    empty = _dev(torch_cuda, np.zeros(16, DTYPE[sb]))[:0]
    r, c, _ = plan.scan_words(empty, ranges=ranges, capacity=16)
    assert int(c.item()) == 0
    r, c, _ = plan.scan_words(_dev(torch_cuda, _sym(b"q" * 3000, sb)), ranges=ranges, capacity=16)
    assert int(c.item()) == 0
    assert plan.scan_words_host(np.zeros(0, DTYPE[sb]), ranges=ranges).size == 0
    plan.status()
    return sym, ranges


def test_fused_calls_on_every_symbol_size_and_a_pending_delta(torch_cuda, novel_bytes):
    keywords, text, rec, want = novel_case(novel_bytes)
    for sb in (1, 2, 4, 8):
        first = 3 if sb == 1 else len(keywords)                     # the byte plan gets its last five keywords as a delta
        m = acm.Machine(sb)
        for kw in keywords[:first]:
            m.add_keyword(_sym(kw, sb))
        plan = m.plan(0)
        if first < len(keywords):
            for kw in keywords[first:]:
                m.add_keyword(_sym(kw, sb))
            plan.update(m)
            assert plan.info.delta_keywords == len(keywords) - first and plan.info.merges == 0, plan.describe()
        sym, ranges = fused_calls_on_plan(torch_cuda, plan, sb, text, rec, want)
        # the machine's own call, on a GPU path
        _same(m.scan_words(sym, ranges=ranges), want)
        assert m.scan_path == PATH_GPU
        with pytest.raises(acm.ACMError):
            m.scan_words(sym, ranges=ranges, capacity=want.size)                        # room for the kept records alone is not enough
        plan.status()


def test_records_that_break_the_contract_are_dropped_and_reported(torch_cuda):
    m, o = build_pair(KEYWORDS, 1)
    rec = oracle_records(KEYWORDS, TEXT)
    want = words(rec, TEXT)
    dev = _dev(torch_cuda, TEXT)
    pos_base = 1000
    shifted, want_shifted = rec.copy(), want.copy()
    shifted["end_pos"] += pos_base
    want_shifted["end_pos"] += pos_base
    bad = {"a start below pos_base": (pos_base + 2, 4, 9), "a length of 0": (pos_base + 20, 0, 9), "beyond the buffer": (pos_base + len(TEXT), 1, 9),
           "below pos_base": (pos_base - 1, 1, 9), "far beyond": (1 << 62, 3, 9)}
    for what, triple in bad.items():
        plan = m.plan(0)
        plan.status()
        mixed = np.concatenate([shifted[:5], np.array([triple], po.RECORD_DTYPE), shifted[5:]])
        _same(_filter(plan, dev, mixed, pos_base=pos_base), want_shifted, what)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_offsets_that_break_the_contract_keep_nothing(torch_cuda):
    torch = torch_cuda
    m, o = build_pair(KEYWORDS, 1)
    rec = oracle_records(KEYWORDS, TEXT)
    dev = _dev(torch, TEXT)
    n = len(TEXT)
    prefilled = _hand_made(np.full(rec.size, PATTERN, np.uint64), 7, 7)
    for what, off in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]), ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n]), *broken_last_pair(n)):
        plan = m.plan(0)
        plan.status()
        d_out = _rec_dev(torch, prefilled)
        out, cnt = plan.words_records(dev, _rec_dev(torch, rec), rec.size, offsets=_dev(torch, np.array(off, np.int64)), out=d_out)
        assert int(cnt.item()) == 0, what
        assert np.array_equal(_rec_host(d_out, rec.size), prefilled), what
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_whole_word_replace_on_the_device(torch_cuda, novel_bytes):
    """scan_words -> select_records -> replace_records, every count read on the device; nothing comes to
    the host before the final compare"""
    torch = torch_cuda
    keywords, text, rec, whole = novel_case(novel_bytes)
    # (the novel sets a tab between its words: with this ninth keyword two whole-word matches overlap and the selection has work)
    keywords = keywords + [b"Mrs.\tDalloway"]
    rec = oracle_records(keywords, text)
    whole = words(rec, text)
    assert as_set(whole) == words_by_re(keywords, text)
    sel = greedy(whole)
    table = [b"HE", b"SHE", b"HIS", b"HERS", b"THE", b"Mr", b"D.", b"Mrs D.", b"Mrs D."]
    want, _ = replace_by_definition(text, sel, table)
    plain, _ = replace_by_definition(text, greedy(rec), table)
    assert 0 < sel.size < whole.size and not np.array_equal(want, plain) and b"HEr" in plain.tobytes() and b"HEr" not in want.tobytes()
    m, o = build_pair(keywords, 1)
    plan = m.plan(0)
    L = acm.lib()
    dev = _dev(torch, text)
    records, count, _ = plan.scan_words(dev, capacity=rec.size)
    tb = L.acm_gpu_select_tmp_bytes(plan.h, rec.size, len(text))
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    assert L.acm_gpu_select_records_device(plan.h, records.data_ptr(), rec.size, count.data_ptr(), 0, len(text), records.data_ptr(), count.data_ptr(),
                                           tmp.data_ptr(), tb, plan._stream()) == 0
    res = plan.replace_records(dev, records, rec.size, replacements=table, count=count)
    assert res.count == sel.size and res.out_symbols == want.size
    assert np.array_equal(res.out[:res.out_symbols].cpu().numpy(), want)
    _same(_rec_host(records, sel.size), sel)
    plan.status()
