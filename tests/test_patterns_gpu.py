"""Keyword patterns with don't-care gaps on the GPU (acm_gpu_patterns_*, acm_gpu_scan_patterns_*,
acm_scan_patterns; csrc/dev_patterns.h).  The expected answer is always the definition of PATTERNS in plain
Python over the ORACLE's records (tests/pattern_cases.py) and, for byte text, a second derivation from the
text alone with `re` lookaheads -- never the library's own scan or join.  All comparisons are exact, order
included.  Texts are a few KiB; one case has more records than the capped grid has tiles of 64, so that
blocks stride over tiles."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import broken_last_pair, offsets_of, oracle_batch
from tests.pattern_cases import as_records, byte_oracle, compile_templates, oracle_records, patterns, patterns_by_re
from tests.tally_cases import PATH_CLASSES, PATH_GPU, kind

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
TEMPLATES = [b"a?c", b"ab?d", b"a?cd", b"b?d", b"a??d", b"?bc"]
TEXT = b"abcd abxd axcd xbc ab aabcdd bcd b?d abbd acc abc"
SENTINEL = 0x0123456789ABCDEF


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
    assert got.size == want.size and np.array_equal(np.asarray(got).astype(po.RECORD_DTYPE), want), (what, got.size, want.size, got[:8], want[:8])


def _sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(DTYPE[sb])


def _join(plan, rec, pats, n_symbols, **kw):
    """Plan.patterns_records on the records `rec` (host): (the matches (host), the count)"""
    torch = __import__("torch")
    out, cnt = plan.patterns_records(_rec_dev(torch, rec), rec.size, pats, n_symbols, **kw)
    n = int(cnt.item())
    return _rec_host(out, min(n, out.shape[0])), n


def _scan(plan, dev, pats, capacity, **kw):
    """Plan.scan_patterns: (the matches (host), the count, the scan's count)"""
    out, cnt, found, _ = plan.scan_patterns(dev, pats, capacity=capacity, **kw)
    n = int(cnt.item())
    return _rec_host(out, min(n, out.shape[0])), n, int(found.item())


def _words(m):
    return [tuple(m.keyword(k)[0]) for k in range(m.nb_keywords)]


def _byte_case(templates=TEMPLATES, text=TEXT, offsets=None):
    """(machine, pattern set, the oracle's records of the text, PATTERNS of them) for byte templates: the two
    derivations must agree before anything else is compared"""
    m = acm.Machine(1)
    ps = binding.PatternSet.from_templates(m, templates, wildcard=b"?")
    kws, pats = compile_templates(templates)
    assert [tuple(k) for k in kws] == _words(m) and ps.terms.tolist() == [list(t) for p in pats for t in p]
    rec = oracle_records([bytes(k) for k in kws], text)
    want = patterns(rec, pats, len(text), offsets)
    _same(want, patterns_by_re(templates, text, offsets), "the two derivations")
    return m, ps, rec, want


def test_the_case_is_not_trivial():
    m, ps, rec, want = _byte_case()
    per = np.bincount(want["keyword_id"], minlength=len(TEMPLATES))
    ties = int(np.count_nonzero(want["end_pos"][1:] == want["end_pos"][:-1]))
    print("records %d, matches per template %s, ties %d" % (rec.size, per.tolist(), ties))
    assert np.all(per >= 2) and ties >= 2


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_templates_on_every_symbol_size(torch_cuda, sb):
    _, _, rec, want = _byte_case()
    m = acm.Machine(sb)
    ps = binding.PatternSet.from_templates(m, [_sym(t, sb) for t in TEMPLATES], wildcard=int(_sym(b"?", sb)[0]))
    assert m.nb_keywords == len(compile_templates(TEMPLATES)[0])
    plan = m.plan(0)
    sym = _sym(TEXT, sb)
    dev = _dev(torch_cuda, sym)
    P = plan.patterns_create(ps)
    info = P.info()
    assert info["patterns"] == len(TEMPLATES) and info["terms"] == ps.terms.shape[0] and info["longest"] == 4 and info["max_anchor_postings"] >= 2
    got, n, found = _scan(plan, dev, P, rec.size)
    assert found == rec.size and n == want.size
    _same(got, want, sb)
    # the join alone on the oracle's records, with the compiled set and with a set compiled for the call
    _same(_join(plan, rec, P, len(TEXT))[0], want, sb)
    _same(_join(plan, rec, ps, len(TEXT))[0], want, sb)
    # nonzero pos_base
    moved, shifted = want.copy(), rec.copy()
    moved["end_pos"] += 5000
    shifted["end_pos"] += 5000
    _same(_scan(plan, dev, P, rec.size, pos_base=5000)[0], moved, sb)
    _same(_join(plan, shifted, P, len(TEXT), pos_base=5000)[0], moved, sb)
    # host memory in, blocking; the machine's own call on a GPU path
    _same(plan.scan_patterns_host(sym, ps), want, sb)
    _same(plan.scan_patterns_host(sym, ps, pos_base=5000), moved, sb)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_patterns_host(sym, ps, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW
    _same(m.scan_patterns(sym, ps), want, sb)
    assert m.scan_path == PATH_GPU
    with pytest.raises(acm.ACMError) as e:
        m.scan_patterns(sym, ps, out_capacity=want.size - 1)
    assert e.value.code == E_OVERFLOW
    wrong = binding.PatternSet([[(0, 0, 2)]])                      # keyword 0 is one symbol long: the machine's call knows
    with pytest.raises(acm.ACMError) as e:
        m.scan_patterns(sym, wrong)
    assert e.value.code == E_ARG
    assert plan.scan_patterns_host(sym, wrong).size == 0           # the plan's call cannot: the term never holds
    # an empty text, a text without a record
    assert plan.scan_patterns_host(np.zeros(0, DTYPE[sb]), ps).size == 0
    got, n, found = _scan(plan, _dev(torch_cuda, _sym(b"q" * 3000, sb)), P, 16)
    assert (n, found) == (0, 0)
    P.close()
    plan.status()


def test_a_class_plan_matches_over_classes(torch_cuda, kat):
    cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
    m, o = acm.Machine(1, cmp=cmp), po.Oracle(1, po.MEYER85, cmp=cmp)
    ps = binding.PatternSet.from_templates(m, TEMPLATES, wildcard=b"?")
    for w in _words(m):
        o.add_keyword(bytes(w))
    m.set_symbol_bytes(1)
    text = b"ABcd aBxD AxCd xBC ab AaBcDd bCD B?d abBD Acc aBc"
    assert text.lower() == TEXT
    rec = o.scan(text)
    want = patterns(rec, compile_templates(TEMPLATES)[1], len(text))
    _same(want, patterns_by_re(TEMPLATES, text.lower()), "the two derivations")
    assert patterns_by_re(TEMPLATES, text).size < want.size         # (the exact-case reading finds fewer)
    plan = m.plan_classes(0)
    got, n, found = _scan(plan, _dev(torch_cuda, text), ps, rec.size)
    assert found == rec.size
    _same(got, want)
    _same(plan.scan_patterns_host(np.frombuffer(text, np.uint8), ps), want)
    _same(m.scan_patterns(text, ps), want)
    assert m.scan_path == PATH_CLASSES
    plan.status()


@pytest.mark.parametrize("name", ["dense", "gram", "starts"])
def test_scan_patterns_on_plan_kinds(torch_cuda, monkeypatch, kat, name):
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    sb = m.sym_size
    before = m.nb_keywords
    wild = 0xFFFFFF if sb == 4 else ord("?")
    templates = [np.frombuffer(t.replace(b"?", b"\xff"), np.uint8).astype(DTYPE[sb]) for t in TEMPLATES]
    for t in templates:
        t[t == 0xFF] = wild
    ps = binding.PatternSet.from_templates(m, templates, wildcard=wild)
    for k in range(before, m.nb_keywords):                          # the oracle gets the new fragments under the same ids
        o.add_keyword(np.array(m.keyword(k)[0], DTYPE[sb]))
    assert o.nb_keywords == m.nb_keywords
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    own = np.frombuffer(TEXT, np.uint8).astype(DTYPE[sb])
    buf = np.concatenate([own, text[:4096].astype(DTYPE[sb]), own])
    rec = o.scan(buf)
    pats = [[tuple(int(x) for x in ps.terms[i]) for i in range(int(ps.pat_ptr[p]), int(ps.pat_ptr[p + 1]))] for p in range(ps.n_patterns)]
    want = patterns(rec, pats, buf.size)
    if sb == 1:
        _same(want, patterns_by_re(TEMPLATES, buf.tobytes()), "the two derivations")
    print("%s: records %d, matches %d" % (name, rec.size, want.size))
    assert want.size >= 2 * _byte_case()[3].size
    got, n, found = _scan(plan, _dev(torch_cuda, buf), ps, rec.size)
    assert found == rec.size
    _same(got, want, name)
    plan.status()


def test_an_interleaved_group_comes_out_in_order(torch_cuda):
    templates = [b"c?e", b"a??de", b"b?de", b"ab??e"]
    m, ps, rec, want = _byte_case(templates, b"abcde")
    assert [tuple(int(x) for x in r) for r in want] == [(4, 5, 1), (4, 5, 3), (4, 4, 2), (4, 3, 0)]
    plan = m.plan(0)
    _same(_join(plan, rec, ps, 5)[0], want)
    _same(_scan(plan, _dev(torch_cuda, b"abcde"), ps, rec.size)[0], want)
    # many such groups side by side, and groups of one between them
    text = b"abcde xbcde abcdeabcde cce " * 40
    m, ps, rec, want = _byte_case(templates, text)
    sizes = np.unique(np.unique(want["end_pos"], return_counts=True)[1])
    assert sizes.tolist() == [1, 2, 4]
    _same(_join(plan, rec, ps, len(text))[0], want)
    plan.status()


def test_a_pile_of_more_than_64_matches_at_one_end(torch_cuda):
    templates = [b"a" + b"?" * k + b"z" for k in range(1, 101)] + [b"aa?z"]
    text = b"a" * 120 + b"z"
    m, ps, rec, want = _byte_case(templates, text)
    assert want.size == 101 and np.all(want["end_pos"] == 120)
    assert [int(x) for x in want["keyword_id"][-4:]] == [2, 1, 100, 0]           # a???z, then a??z in front of aa?z (equal lengths), then a?z
    plan = m.plan(0)
    P = plan.patterns_create(ps)
    assert P.info()["max_anchor_postings"] == 101 and P.info()["anchor_keywords"] == 1 and P.info()["longest"] == 102
    _same(_join(plan, rec, P, len(text))[0], want)
    _same(_scan(plan, _dev(torch_cuda, text), P, rec.size)[0], want)
    # four piles side by side (a don't-care also matches a `z`)
    text = b"a" * 120 + b"z" + b"a" * 30 + b"z" + b"a" * 110 + b"zz"
    m2, ps2, rec, want = _byte_case(templates, text)
    assert sorted(np.unique(want["end_pos"], return_counts=True)[1].tolist()) == [100, 101, 101, 101]
    _same(_join(plan, rec, P, len(text))[0], want)
    plan.status()


def test_text_boundaries_of_a_packed_batch(torch_cuda):
    texts = [b"", b"ab", b"cd", b"abxd", b"xbc", b"", b"", b"a", b"bc", b"abcd abcd", b"", b"bcd", b"ab", b"d", b""] * 12 + [b""]
    packed = b"".join(texts)
    off = offsets_of(texts)
    m, ps, rec, want = _byte_case(TEMPLATES, packed, off)
    o = byte_oracle([bytes(k) for k in compile_templates(TEMPLATES)[0]])
    pats = compile_templates(TEMPLATES)[1]
    whole = patterns(rec, pats, len(packed))
    got_set = {tuple(int(x) for x in r) for r in want}
    whole_set = {tuple(int(x) for x in r) for r in whole}
    # `ab|cd`: a?c, b?d, ab?d, a?cd and a??d would span the cut; `abxd` fills its text; `xbc`: a leading don't-care at a text's first
    # symbol; `a|bc`: the don't-care of ?bc would lie in the text in front
    spanning = {(2, 3, 0), (3, 3, 3), (3, 4, 1), (3, 4, 2), (3, 4, 4), (13, 3, 5)}
    assert spanning <= whole_set and not spanning & got_set
    assert {(7, 3, 3), (7, 4, 1), (7, 4, 4), (10, 3, 5)} <= got_set and 0 < want.size < whole.size
    batch_rec = oracle_batch(o, texts)[0]
    assert batch_rec.size < rec.size
    _same(patterns(batch_rec, pats, len(packed), off), want, "PATTERNS of the batch's records")
    plan = m.plan(0)
    dev, d_off = _dev(torch_cuda, packed), _dev(torch_cuda, off.astype(np.int64))
    _same(_join(plan, rec, ps, len(packed), offsets=d_off)[0], want)
    _same(_join(plan, batch_rec, ps, len(packed), offsets=d_off)[0], want)
    _same(_join(plan, rec, ps, len(packed))[0], whole)
    got, n, found = _scan(plan, dev, ps, rec.size, offsets=d_off)
    assert found == rec.size
    _same(got, want)
    _same(plan.scan_patterns_host(np.frombuffer(packed, np.uint8), ps, offsets=off), want)
    _same(m.scan_patterns(packed, ps, offsets=off), want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_patterns_host(np.frombuffer(packed, np.uint8), ps, offsets=[0, 9, 5, len(packed)])
    assert e.value.code == E_ARG
    plan.status()                                                                       # a record across a cut is no error


def test_more_tiles_than_the_grid_has_blocks(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles"""
    monkeypatch.setenv("ACM_GPU_PATTERNS_TILE", "64")
    templates = [b"a?b", b"b??a", b"ab"]
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus + 3) * 64 + 65
    text = bytes(np.random.default_rng(8).choice(np.frombuffer(b"ab", np.uint8), size=n))
    m = acm.Machine(1)
    ps = binding.PatternSet.from_templates(m, templates, wildcard=b"?")
    kws, pats = compile_templates(templates)
    rec = oracle_records([bytes(k) for k in kws], text)
    assert rec.size > n
    want = patterns_by_re(templates, text)
    _same(patterns(rec[rec["end_pos"] < 3000], pats, 3000), want[want["end_pos"] < 3000], "the two derivations, where the loop is affordable")
    plan = m.plan(0)
    got, cnt = _join(plan, rec, ps, n)
    _same(got, want)
    assert n // 2 < want.size
    plan.status()


def test_out_capacity_counts_on_the_device_and_overflow(torch_cuda):
    torch = torch_cuda
    text = TEXT * 13
    m, ps, rec, want = _byte_case(TEMPLATES, text)
    plan = m.plan(0)
    P = plan.patterns_create(ps)
    dev = _dev(torch, text)
    assert want.size > 64
    sentinel = as_records([(SENTINEL, 7, 7)] * (want.size + 8))

    def join(out_capacity, count=None, room=None):
        d_out = _rec_dev(torch, sentinel)
        d_rec = _rec_dev(torch, rec, room, fill=SENTINEL)
        out, cnt = plan.patterns_records(d_rec, rec.size if room is None else room, P, len(text), out=d_out, out_capacity=out_capacity, count=count)
        return _rec_host(d_out, sentinel.size), int(cnt.item())
    # the exact room; one short: the count is exact and nothing is written at or behind out_capacity; no room: the count alone
    out, n = join(want.size)
    assert n == want.size and np.array_equal(out[want.size:], sentinel[want.size:])
    _same(out[:n], want)
    out, n = join(want.size - 1)
    assert n == want.size and np.array_equal(out[want.size - 1:], sentinel[want.size - 1:])
    out, n = join(0)
    assert n == want.size and np.array_equal(out, sentinel)
    out, n = join(1)
    assert n == want.size and np.array_equal(out[1:], sentinel[1:])
    # d_n given: n is the room of the records
    room = rec.size + 100
    out, n = join(want.size, count=torch.tensor([rec.size], dtype=torch.int64, device="cuda"), room=room)
    _same(out[:n], want)
    # a scan that overflowed: *d_n > room -- *d_count = 0 and nothing is written
    out, n = join(want.size, count=torch.tensor([room + 1], dtype=torch.int64, device="cuda"), room=room)
    assert n == 0 and np.array_equal(out, sentinel)
    # the fused call with too little room for the scan's records: no match, *d_found suffices on repeat
    got, n, found = _scan(plan, dev, P, rec.size - 1, out_capacity=want.size)
    assert n == 0 and found == rec.size
    got, n, found = _scan(plan, dev, P, found, out_capacity=want.size)
    assert found == rec.size
    _same(got, want)
    got, n, found = _scan(plan, dev, P, 0, out_capacity=want.size)                     # no room at all: the scan's count
    assert n == 0 and found == rec.size
    got, n, found = _scan(plan, dev, P, rec.size, out_capacity=want.size - 1)          # the records fit, the matches do not
    assert n == want.size and found == rec.size
    P.close()
    plan.status()


def test_patterns_device_arguments(torch_cuda):
    torch = torch_cuda
    m, ps, rec, want = _byte_case()
    plan = m.plan(0)
    other = acm.Machine(1)
    other.add_keyword(b"q")
    P = plan.patterns_create(ps)
    L = acm.lib()
    d_rec = _rec_dev(torch, rec, 2 * rec.size + want.size)
    sentinel = as_records([(SENTINEL, 7, 7)] * want.size)
    d_out = _rec_dev(torch, sentinel)
    count = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_patterns_tmp_bytes(plan.h, P.h, rec.size, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call(plan_h=plan.h, pat=P.h, records=d_rec.data_ptr(), n=rec.size, out=d_out.data_ptr(), cap=want.size, cnt=count.data_ptr(),
             scratch=tmp.data_ptr(), tmp_bytes=tb, offsets=None, n_texts=0):
        return L.acm_gpu_patterns_records_device(plan_h, pat, records, n, None, len(TEXT), 0, offsets, n_texts, out, cap, cnt, scratch, tmp_bytes, None)
    assert tb > 0 and L.acm_gpu_patterns_tmp_bytes(plan.h, P.h, 1 << 31, 0) == 0 and L.acm_gpu_patterns_tmp_bytes(plan.h, None, 64, 0) == 0
    assert L.acm_gpu_scan_patterns_tmp_bytes(plan.h, P.h, 1 << 31, 64, 0) == 0 and L.acm_gpu_scan_patterns_tmp_bytes(plan.h, P.h, 64, 64, 0) > 0
    assert call(plan_h=None) == E_ARG and call(pat=None) == E_ARG and call(records=None) == E_ARG and call(out=None) == E_ARG
    assert call(cnt=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(cap=1 << 31) == E_ARG
    assert call(out=d_rec.data_ptr()) == E_ARG and call(out=d_rec.data_ptr() + 16 * (rec.size - 1)) == E_ARG     # d_out overlapping d_records
    assert call(out=d_rec.data_ptr() - 16 * (want.size - 1)) == E_ARG
    assert call(offsets=d_rec.data_ptr(), n_texts=0) == E_ARG                          # no text, but symbols
    h = C.c_void_p()
    assert L.acm_gpu_patterns_create(plan.h, *binding.PatternSet([[(m.nb_keywords, 0, 1)]]).args(), C.byref(h)) == E_ARG
    assert L.acm_gpu_patterns_create(None, *ps.args(), C.byref(h)) == E_ARG and L.acm_gpu_patterns_create(plan.h, *ps.args(), None) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(_rec_host(d_out, want.size), sentinel) and int(count.item()) == 0x5A5A                  # nothing was touched
    assert call(out=d_rec.data_ptr() + 16 * rec.size) == 0                             # right behind the records: no overlap
    torch.cuda.synchronize()
    _same(_rec_host(d_rec[rec.size:], int(count.item())), want)
    assert call() == 0
    torch.cuda.synchronize()
    _same(_rec_host(d_out, int(count.item())), want)
    assert call(n=0, records=None, scratch=None, tmp_bytes=0) == 0                      # no record: no match
    torch.cuda.synchronize()
    assert int(count.item()) == 0
    P.close()
    plan.status()


def test_offsets_that_break_the_contract_match_nothing(torch_cuda):
    torch = torch_cuda
    m, ps, rec, want = _byte_case()
    n = len(TEXT)
    sentinel = as_records([(SENTINEL, 7, 7)] * want.size)
    for what, off in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]), ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n]), *broken_last_pair(n)):
        plan = m.plan(0)
        plan.status()
        d_out = _rec_dev(torch, sentinel)
        out, cnt = plan.patterns_records(_rec_dev(torch, rec), rec.size, ps, n, offsets=_dev(torch, np.array(off, np.int64)), out=d_out)
        assert int(cnt.item()) == 0, what
        assert np.array_equal(_rec_host(d_out, want.size), sentinel), what
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_records_that_break_the_contract_are_skipped_and_reported(torch_cuda):
    m, ps, rec, want = _byte_case()
    pos_base = 1000
    shifted, moved = rec.copy(), want.copy()
    shifted["end_pos"] += pos_base
    moved["end_pos"] += pos_base
    d_kw = 3                                                                            # (a keyword that anchors patterns: the record would be looked at)
    bad = {"a start below pos_base": (pos_base + 2, 4, d_kw), "a length of 0": (pos_base + 20, 0, d_kw), "beyond the buffer": (pos_base + len(TEXT), 1, d_kw),
           "below pos_base": (pos_base - 1, 1, d_kw), "far beyond": (1 << 62, 3, d_kw)}
    for what, triple in bad.items():
        plan = m.plan(0)
        plan.status()
        mixed = np.concatenate([shifted, np.array([triple], po.RECORD_DTYPE)])
        mixed = mixed[np.lexsort((-mixed["length"].astype(np.int64), mixed["end_pos"]))]   # canonical order with the stranger in it
        _same(_join(plan, mixed, ps, len(TEXT), pos_base=pos_base)[0], moved, what)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_a_keyword_added_after_plan_creation_is_a_fragment(torch_cuda):
    text = TEXT * 3
    m = acm.Machine(1)
    early = binding.PatternSet.from_templates(m, [b"ab?d"], wildcard=b"?")             # ab, d
    plan = m.plan(0)
    P0 = plan.patterns_create(early)
    ps = binding.PatternSet.from_templates(m, TEMPLATES, wildcard=b"?")                 # more fragments: the machine is ahead of the plan
    with pytest.raises(acm.ACMError) as e:
        plan.patterns_create(ps)
    assert e.value.code == E_ARG                                                        # the plan does not know them yet
    plan.update(m)
    P = plan.patterns_create(ps)
    words = [bytes(w) for w in _words(m)]
    rec = oracle_records(words, text)
    pats = [[tuple(int(x) for x in ps.terms[i]) for i in range(int(ps.pat_ptr[p]), int(ps.pat_ptr[p + 1]))] for p in range(ps.n_patterns)]
    want = patterns(rec, pats, len(text))
    _same(want, patterns_by_re(TEMPLATES, text), "the two derivations")
    dev = _dev(torch_cuda, text)
    got, n, found = _scan(plan, dev, P, rec.size)
    assert found == rec.size
    _same(got, want)
    # the set made before the update stays valid
    _same(_scan(plan, dev, P0, rec.size)[0], patterns_by_re([b"ab?d"], text))
    _same(m.scan_patterns(text, ps), want)
    P.close()
    P0.close()
    plan.status()
