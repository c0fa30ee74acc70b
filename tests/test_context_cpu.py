"""Match contexts without a GPU: acm_context_records (the sequential pass on the host), the Python
wrappers and acm_context on a machine that takes the caller loop on the host
(ACM_SCAN_PATH_CPU_LOOP).  The expected answer is the definition of CONTEXT in plain Python over the
ORACLE's records or hand-made ones (tests/context_cases.py: the window formula, a cover array) and,
for TEXTS | MERGE over lines, the groups the machine's own `grep -F -C` prints."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.context_cases import (BATCH_TEXTS, KEYWORDS, MOST, NONE, batch_case, expected, grep_groups, have_grep, line_offsets, not_vacuous, novel_page, oracle_records)
from tests.words_cases import loop_machine8, sym8

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
PATH_LOOP = 3
SYM = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}
PATTERN = 0xA5


def _sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes, a high byte set in every wider symbol"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(SYM[sb])


def _check(s, exp, text, what=None):
    """a Snippets of numpy arrays against the expectation, array by array"""
    assert s.n_snippets == exp.n_snippets == len(s) and s.out_symbols == exp.out_symbols, (what, s.n_snippets, exp.n_snippets)
    assert np.array_equal(s.snip_lo, exp.snip_lo), what
    assert np.array_equal(s.out_offsets, exp.out_offsets), what
    assert np.array_equal(s.snip_text, exp.snip_text), (what, s.snip_text, exp.snip_text)
    assert np.array_equal(s.rec_snip, exp.rec_snip), what
    assert np.array_equal(s.rec_at, exp.rec_at), what
    if s.out is not None:
        want = exp.out(text)
        assert np.array_equal(s.out, want), what
        for j in (0, exp.n_snippets - 1) if exp.n_snippets else ():
            assert np.array_equal(s[j], want[int(exp.out_offsets[j]):int(exp.out_offsets[j + 1])])


_batch = batch_case


def test_the_issues_figures_on_the_novel(novel_bytes):
    """brute force on the first 4,096 bytes: 124 records, 93 lines; the snippets of four window sizes"""
    text, rec, lines = novel_page(novel_bytes)
    assert rec.size == 124 and lines.size - 1 == 93
    counts = {ba: expected(rec, len(text), None, ba[0], ba[1]).n_snippets for ba in ((0, 0), (3, 5), (8, 8), (40, 40))}
    print(counts)
    assert counts == {(0, 0): 110, (3, 5): 96, (8, 8): 68, (40, 40): 11}


@pytest.mark.parametrize("before,after", [(0, 0), (3, 5), (8, 8), (40, 40), (MOST, MOST), (0, 7), (9, 0)])
def test_one_text_against_the_definition(novel_bytes, before, after):
    text, rec, _ = novel_page(novel_bytes)
    t = np.frombuffer(text, np.uint8)
    exp = expected(rec, len(text), None, before, after)
    if before != MOST:
        not_vacuous(exp, rec.size)
    else:
        assert exp.n_snippets == 1 and exp.out_symbols == len(text)
    _check(binding.context_records(t, rec, before=before, after=after), exp, t, "merge")
    _check(binding.context_records(t, rec, before=before, after=after, merge=False), expected(rec, len(text), None, before, after, merged=False), t, "each")
    # EACH takes any order
    shuffled = rec[np.random.default_rng(3).permutation(rec.size)]
    _check(binding.context_records(t, shuffled, before=before, after=after, merge=False),
           expected(shuffled, len(text), None, before, after, merged=False), t, "each, shuffled")


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_a_batch_in_every_symbol_size(sb):
    packed, off, rec = _batch()
    t = _sym(packed, sb)
    spans = [r for r in rec if int(r["end_pos"]) >= int(off[np.searchsorted(off, int(r["end_pos"]) + 1 - int(r["length"]), "right")])]
    assert len(spans) >= 2                                                     # `she` of "us|hers", twice: windowless
    for texts, before, after in ((False, 0, 0), (False, 2, 3), (False, MOST, MOST), (True, 0, 0), (True, 1, 1), (True, 0, 2), (True, MOST, MOST)):
        for merged in (True, False):
            exp = expected(rec, len(packed), off, before, after, texts, merged)
            if merged and before != MOST:
                not_vacuous(exp, rec.size)
            assert NONE in exp.rec_snip and -1 in exp.rec_at
            got = binding.context_records(t, rec, offsets=off, before=before, after=after, unit="texts" if texts else "symbols", merge=merged)
            _check(got, exp, t, (sb, texts, before, after, merged))
    # "hers" | "he": the windows touch across a boundary -- two snippets under SYMBOLS, one under TEXTS
    sym = expected(rec, len(packed), off, 0, 0)
    tex = expected(rec, len(packed), off, 0, 0, texts=True)
    b = int(off[BATCH_TEXTS.index(b"he")])
    assert b in sym.snip_lo and int(sym.snip_lo[list(sym.snip_lo).index(b) - 1] + sym.lens[list(sym.snip_lo).index(b) - 1]) == b
    assert b not in tex.snip_lo and tex.n_snippets < sym.n_snippets
    # pos_base
    shifted = rec.copy()
    shifted["end_pos"] += 7000
    _check(binding.context_records(t, shifted, offsets=off, before=2, after=3, pos_base=7000), expected(rec, len(packed), off, 2, 3), t)
    # raw bytes with the symbol size beside them
    raw = binding.context_records(t.view(np.uint8), rec, offsets=off, before=2, after=3, sym_size=sb)
    assert np.array_equal(raw.out, expected(rec, len(packed), off, 2, 3).out(t).view(np.uint8)) and np.array_equal(raw[0], raw.out[:int(raw.out_offsets[1]) * sb])


def test_nested_and_touching_windows_without_context():
    """before = after = 0: `he` inside `she` merges with it, and "hehe" touches and is one snippet"""
    text = b"she hehe x he"
    rec = oracle_records(KEYWORDS, text)
    exp = not_vacuous(expected(rec, len(text)), rec.size)
    assert [(int(a), int(n)) for a, n in zip(exp.snip_lo, exp.lens)] == [(0, 3), (4, 4), (11, 2)]
    _check(binding.context_records(np.frombuffer(text, np.uint8), rec), exp, np.frombuffer(text, np.uint8))


@pytest.mark.skipif(not have_grep(), reason="no grep on this machine")
@pytest.mark.parametrize("before,after", [(1, 1), (0, 1), (2, 0)])
def test_texts_merge_over_lines_is_grep_C(novel_bytes, tmp_path, before, after):
    text = novel_bytes[:4096]
    text = text[:text.rindex(b"\n") + 1]
    rec = oracle_records(KEYWORDS, text)
    lines = line_offsets(text)
    groups = grep_groups(KEYWORDS, text, before, after, tmp_path)
    exp = not_vacuous(expected(rec, len(text), lines, before, after, texts=True), rec.size)
    t = np.frombuffer(text, np.uint8)
    assert [bytes(exp.out(t)[int(a):int(b)]) for a, b in zip(exp.out_offsets[:-1], exp.out_offsets[1:])] == groups   # the two derivations agree
    got = binding.context_records(t, rec, offsets=lines, before=before, after=after, unit="texts")
    assert [bytes(got[j]) for j in range(len(got))] == groups
    _check(got, exp, t)


def _call(text, sb, records, offsets=None, before=0, after=0, flags=2, pos_base=0, out_capacity=None, n=None, n_texts=None, gather=True):
    """acm_context_records through ctypes into prefilled arrays: (rc, n_snippets, out_symbols, out, snip_lo, out_offsets)"""
    t = np.ascontiguousarray(text)
    a = np.ascontiguousarray(np.asarray(records, dtype=po.RECORD_DTYPE).reshape(-1))
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    m = a.size if n is None else n
    room = max(a.size, 1)
    out = np.full((t.size if out_capacity is None else out_capacity) * sb + 8, PATTERN, np.uint8)
    snip_lo, out_off = np.full(room, 0xDEAD, np.uint64), np.full(room + 1, 0xDEAD, np.uint64)
    ns, sym = C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    rc = acm.lib().acm_context_records(t.ctypes.data if t.size else None, t.size, sb, pos_base, off.ctypes.data if off is not None else None,
                                       (off.size - 1 if off is not None else 0) if n_texts is None else n_texts, a.ctypes.data if a.size else None, m,
                                       before, after, flags, out.ctypes.data if gather else None, (out.size - 8) // max(sb, 1), C.byref(sym), C.byref(ns),
                                       snip_lo.ctypes.data, out_off.ctypes.data, None, None, None)
    return rc, int(ns.value), int(sym.value), out, snip_lo, out_off


def test_every_argument_rule():
    packed, off, rec = _batch()
    t = np.frombuffer(packed, np.uint8)
    n = len(packed)
    untouched = lambda r: r[1] == 0xDEAD and r[2] == 0xDEAD and (r[3] == PATTERN).all() and (r[4] == 0xDEAD).all() and (r[5] == 0xDEAD).all()
    assert _call(t, 1, rec, off)[0] == 0
    for flags in (4, 5, 8, 1 << 31):
        assert _call(t, 1, rec, off, flags=flags)[0] == E_ARG
    for flags in (1, 3):                                                       # TEXTS without offsets
        r = _call(t, 1, rec, None, flags=flags)
        assert r[0] == E_ARG and untouched(r)
    for sb in (0, 3, 5, 16):
        assert _call(t, sb, rec, off)[0] == E_ARG
    for what, bad_off in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]), ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n])):
        r = _call(t, 1, rec, np.array(bad_off, np.uint64))
        assert r[0] == E_ARG and untouched(r), what
    bad = {"a start below pos_base": (1000 + 2, 4, 9), "a length of 0": (1000 + 20, 0, 9), "beyond the buffer": (1000 + n, 1, 9),
           "below pos_base": (1000 - 1, 1, 9), "far beyond": (1 << 62, 3, 9)}
    shifted = rec.copy()
    shifted["end_pos"] += 1000
    for what, triple in bad.items():
        for flags in (0, 2):
            mixed = np.concatenate([shifted[:5], np.array([triple], po.RECORD_DTYPE), shifted[5:]])
            r = _call(t, 1, mixed, off, pos_base=1000, flags=flags)
            assert r[0] == E_ARG and untouched(r), what
    # MERGE wants end_pos never to decrease; EACH takes the same records
    swapped = rec.copy()
    swapped[[3, 9]] = swapped[[9, 3]]
    assert swapped["end_pos"][3] > swapped["end_pos"][4]
    r = _call(t, 1, swapped, off, flags=2)
    assert r[0] == E_ARG and untouched(r)
    assert _call(t, 1, swapped, off, flags=0)[0] == 0
    ties = np.concatenate([rec[:4], rec[3:4], rec[4:]])                        # an end_pos that stays is no decrease
    assert _call(t, 1, ties, off, flags=2)[0] == 0
    # m or n_texts of 2^31 or more
    assert _call(t, 1, rec, off, n=1 << 31)[0] == E_ARG and _call(t, 1, rec, off, n_texts=1 << 31)[0] == E_ARG
    L = acm.lib()
    ns = C.c_uint64(0)
    assert L.acm_context_records(t.ctypes.data, n, 1, 0, None, 0, rec.ctypes.data, rec.size, 0, 0, 2, None, 0, None, C.byref(ns), None, None, None, None,
                                 None) == E_ARG
    assert L.acm_context_records(t.ctypes.data, n, 1, 0, None, 0, rec.ctypes.data, rec.size, 0, 0, 2, None, 0, C.byref(ns), None, None, None, None, None,
                                 None) == E_ARG
    assert L.acm_context_records(None, n, 1, 0, None, 0, rec.ctypes.data, rec.size, 0, 0, 2, None, 0, C.byref(ns), C.byref(ns), None, None, None, None,
                                 None) == E_ARG
    # no records: no snippet
    r = _call(t, 1, rec[:0], off)
    assert r[:3] == (0, 0, 0) and r[5][0] == 0


def test_output_room():
    packed, off, rec = _batch()
    t = np.frombuffer(packed, np.uint8)
    for flags in (0, 2):
        exp = expected(rec, len(packed), off, 2, 3, merged=flags == 2)
        # out NULL: nothing is gathered, the length is reported whatever the capacity says
        r = _call(t, 1, rec, off, 2, 3, flags, gather=False, out_capacity=0)
        assert r[:3] == (0, exp.n_snippets, exp.out_symbols)
        # one symbol short: the length needed, nothing written to out, every index array valid
        r = _call(t, 1, rec, off, 2, 3, flags, out_capacity=exp.out_symbols - 1)
        assert r[:3] == (E_OVERFLOW, exp.n_snippets, exp.out_symbols) and (r[3] == PATTERN).all()
        assert np.array_equal(r[4][:exp.n_snippets], exp.snip_lo) and np.array_equal(r[5][:exp.n_snippets + 1], exp.out_offsets)
        # exactly enough: nothing behind it is written
        r = _call(t, 1, rec, off, 2, 3, flags, out_capacity=exp.out_symbols)
        assert r[0] == 0 and np.array_equal(r[3][:exp.out_symbols], exp.out(t)) and (r[3][exp.out_symbols:] == PATTERN).all()
    with pytest.raises(acm.ACMError) as e:
        binding.context_records(t, rec, offsets=off, before=2, after=3, out_capacity=5)
    assert e.value.code == E_OVERFLOW
    s = binding.context_records(t, rec, offsets=off, before=2, after=3, gather=False)
    assert s.out is None and s.out_symbols == expected(rec, len(packed), off, 2, 3).out_symbols
    with pytest.raises(IndexError):
        s[0]


def _context(h, text8, capacity, before, after, flags, out_capacity, records=True):
    t = np.ascontiguousarray(text8)
    rec = np.zeros(max(capacity, 1), po.RECORD_DTYPE)
    out = np.full(max(out_capacity, 1), PATTERN, np.uint64)
    snip_lo, out_off = np.zeros(max(capacity, 1), np.uint64), np.zeros(capacity + 1, np.uint64)
    rec_snip, rec_at = np.zeros(max(capacity, 1), np.uint32), np.zeros(max(capacity, 1), np.int64)
    n, ns, sym = C.c_uint64(0), C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    rc = acm.lib().acm_context(h, t.ctypes.data, t.size, rec.ctypes.data if records else None, capacity, C.byref(n), before, after, flags,
                               out.ctypes.data, out_capacity, C.byref(sym), C.byref(ns), snip_lo.ctypes.data, out_off.ctypes.data, None,
                               rec_snip.ctypes.data, rec_at.ctypes.data)
    return rc, int(n.value), int(ns.value), int(sym.value), rec, out, snip_lo, out_off, rec_snip, rec_at


def test_acm_context_on_the_host_loop(novel_bytes):
    L = acm.lib()
    text, rec, _ = novel_page(novel_bytes)
    t8 = sym8(text)
    h, keep = loop_machine8(KEYWORDS)
    assert L.acm_scan_path(h) == 0
    for flags in (2, 0):
        exp = not_vacuous(expected(rec, len(text), None, 8, 8), rec.size) if flags else expected(rec, len(text), None, 8, 8, merged=False)
        for records in (True, False):
            rc, n, ns, sym, got_rec, out, snip_lo, out_off, rec_snip, rec_at = _context(h, t8, rec.size, 8, 8, flags, exp.out_symbols, records)
            assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP and (n, ns, sym) == (rec.size, exp.n_snippets, exp.out_symbols)
            assert not records or np.array_equal(got_rec[:n], rec)
            assert np.array_equal(out[:sym], exp.out(t8)) and np.array_equal(snip_lo[:ns], exp.snip_lo) and np.array_equal(out_off[:ns + 1], exp.out_offsets)
            assert np.array_equal(rec_snip[:n], exp.rec_snip) and np.array_equal(rec_at[:n], exp.rec_at)
    exp = expected(rec, len(text), None, 8, 8)
    # the two overflows, told apart by *n_found; the path is recorded on either
    h2, keep2 = loop_machine8(KEYWORDS)
    r = _context(h2, t8, rec.size - 1, 8, 8, 2, exp.out_symbols)
    assert r[0] == E_OVERFLOW and r[1] == rec.size and L.acm_scan_path(h2) == PATH_LOOP and (r[5] == PATTERN).all()
    h3, keep3 = loop_machine8(KEYWORDS)
    r = _context(h3, t8, rec.size, 8, 8, 2, exp.out_symbols - 1)
    assert r[0] == E_OVERFLOW and r[1:4] == (rec.size, exp.n_snippets, exp.out_symbols) and L.acm_scan_path(h3) == PATH_LOOP
    assert (r[5] == PATTERN).all() and np.array_equal(r[6][:exp.n_snippets], exp.snip_lo) and np.array_equal(r[8][:rec.size], exp.rec_snip)
    # one text: TEXTS is refused, and so are flags above 3 and missing counters
    for flags in (1, 3, 4):
        assert _context(h, t8, rec.size, 8, 8, flags, exp.out_symbols)[0] == E_ARG
    n = C.c_uint64(0)
    assert L.acm_context(None, t8.ctypes.data, t8.size, None, 8, C.byref(n), 0, 0, 2, None, 0, C.byref(n), C.byref(n), None, None, None, None, None) == E_ARG
    assert L.acm_context(h, t8.ctypes.data, t8.size, None, 8, None, 0, 0, 2, None, 0, C.byref(n), C.byref(n), None, None, None, None, None) == E_ARG
    assert L.acm_context(h, t8.ctypes.data, t8.size, None, 1 << 31, C.byref(n), 0, 0, 2, None, 0, C.byref(n), C.byref(n), None, None, None, None, None) == E_ARG
    for x in (h, h2, h3):
        L.acm_release(x)


def test_the_exports_and_the_wrappers_call_shape(novel_bytes):
    """what Machine.context runs, on the host loop (a comparator that is none of the GPU's): both rooms grow once"""
    L = acm.lib()
    for name in ("acm_context_records", "acm_gpu_context_tmp_bytes", "acm_gpu_context_records_device", "acm_gpu_scan_context_tmp_bytes",
                 "acm_gpu_scan_context_device", "acm_gpu_scan_context_host", "acm_context"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
    assert (acm.ACM_CONTEXT_SYMBOLS, acm.ACM_CONTEXT_TEXTS, acm.ACM_CONTEXT_EACH, acm.ACM_CONTEXT_MERGE, acm.ACM_CONTEXT_NONE) == (0, 1, 0, 2, NONE)
    assert acm.Snippets is binding.Snippets and acm.context_records is binding.context_records
    for name in ("context_records", "scan_context", "scan_context_host", "grep_context_lines"):
        assert callable(getattr(acm.Plan, name))
    assert callable(acm.Machine.context)
    text, rec, _ = novel_page(novel_bytes)
    # the binding's call shape, on the machine of 8-byte symbols that takes the loop
    h, keep = loop_machine8(KEYWORDS)
    t8 = sym8(text)
    call = binding._context_scan_call(L.acm_context, (h,), t8, t8.size, (), 3, 5, 2)
    s = binding._context_host_call(call, "acm_context", t8, 8, 16, True, True, None)           # both rooms begin too small
    exp = not_vacuous(expected(rec, len(text), None, 3, 5), rec.size)
    _check(s, exp, t8)
    assert np.array_equal(s.records, rec) and s.count == rec.size and L.acm_scan_path(h) == PATH_LOOP
    with pytest.raises(acm.ACMError) as e:
        binding._context_host_call(call, "acm_context", t8, 8, 16, False, True, None)
    assert e.value.code == E_OVERFLOW
    L.acm_release(h)
