"""Whole-word matches without a GPU: acm_words_records (the sequential pass on the host), acm_scan_words
on a machine that takes the caller loop on the host (ACM_SCAN_PATH_CPU_LOOP) and the composition with
the host select and replace passes.  The expected answer is the definition of WORDS in plain Python
over the ORACLE's records (tests/words_cases.py), cross-checked there against Python's `re`."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.words_cases import (ASCII_WORD, BOTH, LEFT, RIGHT, as_set, loop_machine8, novel_case, oracle_records, sym8, words, words_by_re)

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
PATH_LOOP = 3
SYM = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
KEYWORDS = [b"he", b"she", b"his", b"hers", b"the", b"e.g.", b"New York", b"x"]
TEXT = b"the she he, her hers_he e.g. New York's New York x xx ax x_ _x (x) ushers e.g.x his"


# the ASCII word set cut into 16 ranges, a busy one (s-t) last
SIXTEEN = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F)] + [(c, c + 1) for c in range(0x61, 0x7B, 2) if c != 0x73] + [(0x73, 0x74)]
assert len(SIXTEEN) == 16


def _same(got, want):
    assert got.size == want.size and np.array_equal(got.astype(po.RECORD_DTYPE), want), (got[:8], want[:8])


def _call(text, sb, records, offsets=None, ranges=ASCII_WORD, flags=BOTH, pos_base=0, n_symbols=None, n_ranges=None):
    """acm_words_records through ctypes on a copy of `records`: (rc, n_kept, the array afterwards)"""
    t = np.ascontiguousarray(text)
    r = np.ascontiguousarray(np.asarray(ranges, np.uint64).reshape(-1), dtype=SYM.get(sb, np.uint8))
    a = np.array(records, dtype=po.RECORD_DTYPE, copy=True).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64) if offsets is not None else None
    n = C.c_uint64(0xDEAD)
    rc = acm.lib().acm_words_records(t.ctypes.data if t.size else None, t.size if n_symbols is None else n_symbols, sb, pos_base,
                                     off.ctypes.data if off is not None else None, off.size - 1 if off is not None else 0, r.ctypes.data,
                                     r.size // 2 if n_ranges is None else n_ranges, flags, a.ctypes.data if a.size else None, a.size, C.byref(n))
    return rc, int(n.value), a


def test_the_two_derivations_agree_on_the_novel(novel_bytes):
    keywords, text, rec, want = novel_case(novel_bytes)
    _same(binding.words_records(np.frombuffer(text, np.uint8), rec), want)
    for name, flags in (("left", LEFT), ("right", RIGHT), ("both", BOTH)):
        got = binding.words_records(np.frombuffer(text, np.uint8), rec, flags=name)
        assert as_set(got) == words_by_re(keywords, text, flags)
        _same(got, words(rec, text, flags=flags))


def test_flags_symbol_sizes_and_pos_base():
    rec = oracle_records(KEYWORDS, TEXT)
    by_flag = {f: words(rec, TEXT, flags=f) for f in (LEFT, RIGHT, BOTH)}
    assert as_set(by_flag[BOTH]) == words_by_re(KEYWORDS, TEXT)
    sizes = {f: by_flag[f].size for f in by_flag}
    assert 0 < sizes[BOTH] < min(sizes[LEFT], sizes[RIGHT]) and sizes[LEFT] != sizes[RIGHT] and max(sizes.values()) < rec.size, sizes
    # a keyword of non-word symbols and one with a blank inside are whole words by their neighbours alone
    assert {2, 5, 6} <= set(int(k) for k in by_flag[BOTH]["keyword_id"])
    for sb in (1, 2, 4, 8):
        # the letter c as a symbol of sb bytes: the high bytes are set, so that a compare of the low byte alone would be seen
        high = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}[sb]
        text = (np.frombuffer(TEXT, np.uint8).astype(np.uint64) | np.uint64(high)).astype(SYM[sb])
        ranges = [(lo | high, hi | high) for lo, hi in ASCII_WORD]
        for flags in (LEFT, RIGHT, BOTH):
            rc, n, a = _call(text, sb, rec, ranges=ranges, flags=flags)
            assert rc == 0
            _same(a[:n], by_flag[flags])
            shifted = rec.copy()
            shifted["end_pos"] += 1000
            rc, n, a = _call(text, sb, shifted, ranges=ranges, flags=flags, pos_base=1000)
            assert rc == 0
            want = by_flag[flags].copy()
            want["end_pos"] += 1000
            _same(a[:n], want)
        if sb > 1:  # the ASCII ranges themselves hold none of these symbols: everything is whole-word
            rc, n, a = _call(text, sb, rec)
            assert rc == 0 and n == rec.size
    rc, n, a = _call(np.frombuffer(TEXT, np.uint8), 1, rec, ranges=SIXTEEN)
    assert rc == 0
    _same(a[:n], by_flag[BOTH])
    assert words(rec, TEXT, ranges=SIXTEEN[:15]).size != n                       # the sixteenth range counts


def test_offsets_empty_texts_and_records_across_a_cut():
    packed = b"the" + b"he" + b"hers" + b"us" + b"hers" + b"x"
    off = [0, 0, 3, 3, 3, 5, 9, 11, 15, 16, 16]
    rec = oracle_records(KEYWORDS, packed)
    want = words(rec, packed, offsets=off)
    # `he` of "the|he|hers" is a whole text: kept, though both neighbours across the cuts are word symbols;
    # `she` of "us|hers" spans a cut: dropped, whatever its neighbours
    assert {(4, 2, 0), (8, 4, 3), (14, 4, 3), (15, 1, 7)} <= as_set(want) and (12, 3, 1) in as_set(rec) and (12, 3, 1) not in as_set(want)
    crossing = [r for r in rec if not any(off[t] <= int(r["end_pos"]) + 1 - int(r["length"]) and int(r["end_pos"]) < off[t + 1] for t in range(len(off) - 1))]
    assert crossing, "a record of the packed buffer spans a cut"
    for flags in (LEFT, RIGHT, BOTH):
        rc, n, a = _call(np.frombuffer(packed, np.uint8), 1, rec, offsets=off, flags=flags)
        assert rc == 0
        _same(a[:n], words(rec, packed, offsets=off, flags=flags))
    # the same as the per-text answers side by side
    per_text = set()
    for t in range(len(off) - 1):
        piece = packed[off[t]:off[t + 1]]
        per_text |= {(e + off[t], l, k) for e, l, k in words_by_re(KEYWORDS, piece)}
    assert as_set(want) == per_text
    assert as_set(want) != as_set(words(rec, packed))


def test_shuffled_input_keeps_its_order_and_the_smallest_sets():
    rec = oracle_records(KEYWORDS, TEXT)
    rng = np.random.default_rng(1975)
    shuffled = rec[rng.permutation(rec.size)]
    rc, n, a = _call(np.frombuffer(TEXT, np.uint8), 1, shuffled)
    assert rc == 0
    want = words(shuffled, TEXT)
    _same(a[:n], want)
    assert not np.array_equal(want, words(rec, TEXT)) and as_set(want) == as_set(words(rec, TEXT))
    rc, n, a = _call(np.frombuffer(TEXT, np.uint8), 1, np.zeros(0, po.RECORD_DTYPE))
    assert (rc, n) == (0, 0)
    rc, n, a = _call(np.zeros(0, np.uint8), 1, np.zeros(0, po.RECORD_DTYPE), offsets=[0])
    assert (rc, n) == (0, 0)
    # records at symbol 0 and at n - 1: the symbols outside the buffer are not looked at
    text = b"he she"
    rec = oracle_records(KEYWORDS, text)
    rc, n, a = _call(np.frombuffer(text, np.uint8), 1, rec)
    assert rc == 0 and as_set(a[:n]) == {(1, 2, 0), (5, 3, 1)}


def test_every_argument_error_and_nothing_modified():
    text = np.frombuffer(TEXT, np.uint8)
    rec = oracle_records(KEYWORDS, TEXT)

    def refused(**kw):
        records = kw.pop("records", rec)
        sb = kw.pop("sb", 1)
        rc, n, a = _call(kw.pop("text", text), sb, records, **kw)
        assert rc == E_ARG and np.array_equal(a, np.asarray(records, po.RECORD_DTYPE))

    refused(flags=0)
    refused(flags=4)
    refused(n_ranges=0)
    refused(ranges=[(c, c) for c in range(17)])
    refused(ranges=[(0x30, 0x39), (0x7A, 0x61)])
    for sb in (0, 3, 5, 16):
        refused(sb=sb, text=np.zeros(16 * len(TEXT), np.uint8), n_symbols=len(TEXT))
    refused(offsets=[1, len(TEXT)])
    refused(offsets=[0, len(TEXT) - 1])
    refused(offsets=[0, 9, 7, len(TEXT)])
    bad = rec.copy()
    bad["length"][3] = 0
    refused(records=bad)
    bad = rec.copy()
    bad["end_pos"][rec.size - 1] = len(TEXT)
    refused(records=bad)
    bad = rec.copy()
    bad["length"][0] = int(bad["end_pos"][0]) + 2        # a start below the buffer
    refused(records=bad)
    refused(pos_base=1)                                  # record 0 ends at pos_base, its start lies in front
    refused(pos_base=int(rec["end_pos"].max()) + 1)
    n = C.c_uint64(0)
    L = acm.lib()
    r = np.asarray(ASCII_WORD, np.uint8).reshape(-1)
    a = rec.copy()
    assert L.acm_words_records(text.ctypes.data, text.size, 1, 0, None, 0, r.ctypes.data, 4, 3, a.ctypes.data, a.size, None) == E_ARG
    assert L.acm_words_records(None, text.size, 1, 0, None, 0, r.ctypes.data, 4, 3, a.ctypes.data, a.size, C.byref(n)) == E_ARG
    assert L.acm_words_records(text.ctypes.data, text.size, 1, 0, None, 0, None, 4, 3, a.ctypes.data, a.size, C.byref(n)) == E_ARG
    assert L.acm_words_records(text.ctypes.data, text.size, 1, 0, None, 0, r.ctypes.data, 4, 3, None, a.size, C.byref(n)) == E_ARG
    # the plan-level calls refuse a missing plan before they touch a device
    assert L.acm_gpu_words_records_device(None, None, 0, 0, None, 0, r.ctypes.data, 4, 3, None, 0, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_words_device(None, None, 0, 0, None, 0, r.ctypes.data, 4, 3, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_words_host(None, text.ctypes.data, 1, 0, None, 0, r.ctypes.data, 4, 3, a.ctypes.data, 4, C.byref(n)) == E_ARG
    assert L.acm_gpu_words_tmp_bytes(None, 16, 1) == 0 and L.acm_gpu_scan_words_tmp_bytes(None, 16, 16, 1) == 0
    assert L.acm_scan_words(None, text.ctypes.data, 1, r.ctypes.data, 4, 3, a.ctypes.data, 4, C.byref(n)) == E_ARG


def _scan_words(h, text8, capacity, ranges=ASCII_WORD, flags=BOTH):
    t = text8 if text8.size else np.zeros(1, np.uint64)
    r = np.asarray(ranges, np.uint64).reshape(-1)
    out = np.zeros(max(capacity, 1), po.RECORD_DTYPE)
    n = C.c_uint64(0xDEAD)
    rc = acm.lib().acm_scan_words(h, t.ctypes.data, text8.size, r.ctypes.data, r.size // 2, flags, out.ctypes.data, capacity, C.byref(n))
    return rc, int(n.value), out


def test_acm_scan_words_on_the_host_loop(novel_bytes):
    L = acm.lib()
    keywords, text, rec, want = novel_case(novel_bytes)
    h, keep = loop_machine8(keywords)
    assert L.acm_scan_path(h) == 0
    rc, n, out = _scan_words(h, sym8(text), rec.size)
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    _same(out[:n], want)
    for flags in (LEFT, RIGHT):
        rc, n, out = _scan_words(h, sym8(text), rec.size, flags=flags)
        assert rc == 0
        _same(out[:n], words(rec, text, flags=flags))
    # too little room for ALL matches: the count that suffices comes back, the repeat succeeds
    rc, n, out = _scan_words(h, sym8(text), rec.size - 1)
    assert rc == E_OVERFLOW and n == rec.size
    rc, n, out = _scan_words(h, sym8(text), n)
    assert rc == 0
    _same(out[:n], want)
    rc, n, out = _scan_words(h, sym8(b""), 4)
    assert (rc, n) == (0, 0)
    assert _scan_words(h, sym8(text), rec.size, flags=0)[0] == E_ARG
    assert _scan_words(h, sym8(text), rec.size, ranges=[(9, 1)])[0] == E_ARG
    L.acm_release(h)


def test_machine_scan_words_on_the_host_loop_needs_a_symbol_size_of_1_2_4_or_8():
    from tests.tally_cases import loop_machine, sym3
    L = acm.lib()
    h, keep = loop_machine([b"he"])
    t = np.frombuffer(sym3(b"the he"), np.uint8).copy()
    r = np.asarray(ASCII_WORD, np.uint8).reshape(-1)
    out = np.zeros(8, po.RECORD_DTYPE)
    n = C.c_uint64(0)
    assert L.acm_scan_words(h, t.ctypes.data, 6, r.ctypes.data, 4, 3, out.ctypes.data, 8, C.byref(n)) == E_ARG
    L.acm_release(h)


def test_whole_word_replace_is_words_then_select_then_replace():
    keywords = [b"he", b"she", b"his", b"hers"]
    text = b"the she he, her he"
    rec = oracle_records(keywords, text)
    t = np.frombuffer(text, np.uint8)
    whole = binding.words_records(t, rec)
    _same(whole, words(rec, text))
    sel = binding.select_records(whole)
    table = [b"HE", b"she", b"his", b"hers"]
    out = binding.replace_records(t, sel, replacements=table)
    assert bytes(out) == b"the she HE, her HE"
    plain = binding.replace_records(t, binding.select_records(rec), replacements=table)
    assert bytes(plain) == b"tHE she HE, HEr HE" and bytes(plain) != bytes(out)


def test_library_exports_the_words_symbols():
    L = acm.lib()
    for name in ("acm_words_records", "acm_gpu_words_tmp_bytes", "acm_gpu_words_records_device", "acm_gpu_scan_words_tmp_bytes",
                 "acm_gpu_scan_words_device", "acm_gpu_scan_words_host", "acm_scan_words"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
    assert acm.ASCII_WORD == ASCII_WORD and (acm.ACM_WORDS_LEFT, acm.ACM_WORDS_RIGHT, acm.ACM_WORDS_BOTH) == (LEFT, RIGHT, BOTH)
