"""Tokenising without a GPU: acm_tokens_records (the sequential pass on the host) and acm_tokenize on a
machine that takes the caller loop on the host (ACM_SCAN_PATH_CPU_LOOP).  The expected stream is the
definition in plain Python over select_cases.greedy of the ORACLE's records (tests/token_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, TEXTS, offsets_of
from tests.select_cases import random_case
from tests.tally_cases import PATH_LOOP, byte_oracle, loop_machine, sym3
from tests.token_cases import DROP, MODES, RUN, SYMBOL, oracle_case, selection_of, tokens_by_definition

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
USHERS = [b"he", b"she", b"his", b"hers"]
GB = 1000


def _text(b):
    return np.frombuffer(bytes(b), np.uint8)


def _same(tok, want):
    ids, starts, lens, first = want
    assert tok.n_tokens == ids.size
    assert np.array_equal(tok.ids, ids), (tok.ids[:16], ids[:16])
    assert np.array_equal(tok.start, starts) and np.array_equal(tok.length, lens)
    if first is None:
        assert tok.first is None
    else:
        assert np.array_equal(tok.first, first), (tok.first[:16], first[:16])


def test_ushers_as_one_text():
    o = byte_oracle(USHERS)
    rec, sel = oracle_case(o, b"ushers")
    assert sel.size == 1 and int(sel[0]["keyword_id"]) == 1                  # `she` alone, symbols 1 to 3
    want = {SYMBOL: ([GB + ord("u"), 1, GB + ord("r"), GB + ord("s")], [0, 1, 4, 5], [1, 3, 1, 1]),
            RUN: ([GB, 1, GB], [0, 1, 4], [1, 3, 2]),
            DROP: ([1], [1], [3])}
    for mode in MODES:
        ids, starts, lens, first = tokens_by_definition(b"ushers", sel, mode, GB)
        assert (ids.tolist(), starts.tolist(), lens.tolist()) == want[mode] and first is None   # the definition, by hand
        _same(binding.tokens_records(_text(b"ushers"), sel, mode=mode, gap_base=GB), (ids, starts, lens, None))


def test_ushers_as_the_batch_us_hers():
    o = byte_oracle(USHERS)
    off = np.array([0, 2, 6], np.uint64)
    rec, sel = selection_of(o, b"ushers", off)
    assert rec.size == 2 and sel.size == 1 and int(sel[0]["keyword_id"]) == 3 and int(sel[0]["end_pos"]) == 5   # he and hers; SELECT keeps hers
    ids, starts, lens, first = tokens_by_definition(b"ushers", sel, RUN, GB, offsets=off)
    assert (ids.tolist(), starts.tolist(), lens.tolist(), first.tolist()) == ([GB, 3], [0, 2], [2, 4], [0, 1, 2])
    for mode in MODES:
        want = tokens_by_definition(b"ushers", sel, mode, GB, offsets=off)
        _same(binding.tokens_records(_text(b"ushers"), sel, off, mode=mode, gap_base=GB), want)
    tok = binding.tokens_records(_text(b"ushers"), sel, off, mode="symbol", gap_base=GB)
    assert tok.ids.tolist() == [GB + ord("u"), GB + ord("s"), 3] and tok.first.tolist() == [0, 2, 3]
    assert binding.tokens_records(_text(b"ushers"), sel, off, mode="drop").first.tolist() == [0, 0, 1]


def test_abcd_without_a_match():
    none = np.zeros(0, po.RECORD_DTYPE)
    off = np.array([0, 2, 4], np.uint64)
    tok = binding.tokens_records(_text(b"abcd"), none, off, mode=RUN, gap_base=GB)
    assert (tok.ids.tolist(), tok.start.tolist(), tok.length.tolist(), tok.first.tolist()) == ([GB, GB], [0, 2], [2, 2], [0, 1, 2])
    tok = binding.tokens_records(_text(b"abcd"), none, mode=RUN, gap_base=GB)
    assert (tok.ids.tolist(), tok.start.tolist(), tok.length.tolist(), tok.first) == ([GB], [0], [4], None)
    for mode in MODES:
        for offsets in (None, off):
            _same(binding.tokens_records(_text(b"abcd"), none, offsets, mode=mode, gap_base=GB),
                  tokens_by_definition(b"abcd", none, mode, GB, offsets=offsets))
    assert binding.tokens_records(_text(b"abcd"), none, mode=DROP).n_tokens == 0


def test_aa_aaa_on_a_thousand_a():
    text = b"a" * 1000
    rec, sel = oracle_case(byte_oracle([b"aa", b"aaa"]), text)
    assert sel.size == 333
    for mode, n in ((SYMBOL, 334), (RUN, 334), (DROP, 333)):                 # 333 match tokens and one gap symbol
        want = tokens_by_definition(text, sel, mode, GB)
        assert want[0].size == n and np.count_nonzero(want[0] == 1) == 333
        _same(binding.tokens_records(_text(text), sel, mode=mode, gap_base=GB), want)
        if mode != DROP:
            assert int(want[2].sum()) == 1000 and want[1][-1] == 999


def test_batch_cases_and_the_tok_of_mapping():
    o = byte_oracle(KEYWORDS)
    texts = TEXTS + [b"qq", b"qq"]                                           # (a run cut by a boundary between two texts)
    off = offsets_of(texts)
    whole = b"".join(texts)
    rec, sel = oracle_case(o, whole, off)
    tok_of = np.array([70000, 7, 4000000000, 7], np.uint32)                  # two keywords share a vocabulary id
    for mode in MODES:
        for table in (None, tok_of):
            want = tokens_by_definition(whole, sel, mode, GB, table, off)
            _same(binding.tokens_records(_text(whole), sel, off, mode=mode, gap_base=GB, tok_of=table), want)
            assert want[3][0] == 0 and want[3][-1] == want[0].size
            if mode != DROP:
                assert int(want[2].sum()) == len(whole)
    # pos_base: the records' coordinate
    shifted = sel.copy()
    shifted["end_pos"] += np.uint64(1 << 40)
    want = tokens_by_definition(whole, shifted, RUN, GB, tok_of, off, pos_base=1 << 40)
    _same(binding.tokens_records(_text(whole), shifted, off, mode=RUN, gap_base=GB, tok_of=tok_of, pos_base=1 << 40), want)
    assert int(want[1][0]) == 1 << 40


def test_random_cases():
    rng = np.random.default_rng(1975)
    some = 0
    for _ in range(150):
        keywords, text = random_case(rng, 8, 6, int(rng.integers(1, 301)))
        cuts = np.sort(rng.integers(0, len(text) + 1, size=int(rng.integers(0, 12))))
        off = np.concatenate([[0], cuts, [len(text)]]).astype(np.uint64)
        for offsets in (None, off):
            rec, sel = selection_of(byte_oracle(keywords), text, offsets)
            for mode in MODES:
                _same(binding.tokens_records(_text(text), sel, offsets, mode=mode, gap_base=5), tokens_by_definition(text, sel, mode, 5, offsets=offsets))
            some += 0 < sel.size < rec.size
    assert some > 150


def test_two_byte_symbols_are_read_little_endian():
    text = np.array([0x0102, 0xFFFF, 0x0061, 0x0062], np.uint16)
    sel = np.array([(2, 1, 0)], po.RECORD_DTYPE)
    tok = binding.tokens_records(text, sel, mode=SYMBOL, gap_base=(1 << 32) - (1 << 16))
    assert tok.ids.tolist() == [(1 << 32) - (1 << 16) + 0x0102, (1 << 32) - 1, 0, (1 << 32) - (1 << 16) + 0x62]
    tok = binding.tokens_records(text.view(np.uint8), sel, mode=RUN, gap_base=9, sym_size=2)      # raw bytes of 2-byte symbols
    assert (tok.ids.tolist(), tok.start.tolist(), tok.length.tolist()) == ([9, 0, 9], [0, 2, 3], [2, 1, 1])


def _raw(text, rec, mode, cap, off=None, tok_of=None, nk=0, gap_base=0, sb=1, ids=True, first=True, n_texts=None):
    """the C call itself: (rc, n_tokens, ids, starts, lens, first), the arrays with 4 canary entries behind the capacity"""
    L = acm.lib()
    t = np.frombuffer(bytes(text), np.uint8).copy() if len(text) else np.zeros(1, np.uint8)
    r = np.ascontiguousarray(rec, dtype=po.RECORD_DTYPE)
    o = np.asarray(off, np.uint64) if off is not None else None
    k = (o.size - 1 if o is not None else 0) if n_texts is None else n_texts
    a = np.full(cap + 4, 0xA5A5A5A5, np.uint32)
    b = np.full(cap + 4, 0xA5A5A5A5, np.uint64)
    c = np.full(cap + 4, 0xA5A5A5A5, np.uint32)
    f = np.full((o.size if o is not None else 1), 0xA5A5A5A5, np.uint64)
    table = np.asarray(tok_of, np.uint32) if tok_of is not None else None
    need = C.c_uint64(0xDEAD)
    rc = L.acm_tokens_records(t.ctypes.data, len(text) // sb, sb, 0, r.ctypes.data if r.size else None, r.size, o.ctypes.data if o is not None else None,
                              k, table.ctypes.data if table is not None else None, nk, gap_base, mode, a.ctypes.data if ids else None,
                              b.ctypes.data if ids else None, c.ctypes.data if ids else None, cap, C.byref(need),
                              f.ctypes.data if first and o is not None else None)
    return rc, int(need.value), a, b, c, f


def _untouched(*arrays):
    return all(np.all(x == 0xA5A5A5A5) for x in arrays)


def test_count_only_and_capacity_one_short():
    o = byte_oracle(KEYWORDS)
    off = offsets_of(TEXTS)
    whole = b"".join(TEXTS)
    rec, sel = selection_of(o, whole, off)
    for mode in MODES:
        ids, starts, lens, first = tokens_by_definition(whole, sel, mode, 77, offsets=off)
        n = ids.size
        rc, need, a, b, c, f = _raw(whole, sel, mode, 0, off, gap_base=77, ids=False)             # count only: the capacity is ignored
        assert (rc, need) == (0, n) and _untouched(a, b, c) and np.array_equal(f, first)
        rc, need, a, b, c, f = _raw(whole, sel, mode, n - 1, off, gap_base=77)                    # one short
        assert (rc, need) == (E_OVERFLOW, n) and _untouched(a, b, c) and np.array_equal(f, first)
        rc, need, a, b, c, f = _raw(whole, sel, mode, n, off, gap_base=77)                        # exact
        assert (rc, need) == (0, n) and np.array_equal(a[:n], ids) and np.array_equal(b[:n], starts) and np.array_equal(c[:n], lens)
        assert _untouched(a[n:], b[n:], c[n:]) and np.array_equal(f, first)
        rc, need, a, b, c, f = _raw(whole, sel, mode, n, off, gap_base=77, first=False)           # tok_first is optional
        assert (rc, need) == (0, n) and np.array_equal(a[:n], ids) and _untouched(f)
    rc, need, a, b, c, f = _raw(b"", np.zeros(0, po.RECORD_DTYPE), RUN, 4, [0, 0, 0])              # an empty buffer of two empty texts
    assert (rc, need) == (0, 0) and _untouched(a, b, c) and f.tolist() == [0, 0, 0]


@pytest.mark.parametrize("records,nk", [
    ([(3, 3, 0), (4, 2, 0)], 1),        # overlapping
    ([(5, 2, 0), (2, 2, 0)], 1),        # out of order
    ([(6, 2, 0)], 1),                   # beyond the text
    ([(1, 3, 0)], 1),                   # begins in front of it
    ([(2, 0, 0)], 1),                   # no length
    ([(2, 2, 1)], 1),                   # a keyword id out of range of tok_of
])
def test_bad_records_are_refused(records, nk):
    rec = np.array(records, po.RECORD_DTYPE)
    for mode in MODES:
        rc, need, a, b, c, f = _raw(b"abcdef", rec, mode, 16, tok_of=[5], nk=nk)
        assert rc == E_ARG and _untouched(a, b, c)
        if records[0][2] == 0:                                                # without a table the tiling is checked all the same
            assert _raw(b"abcdef", rec, mode, 16)[0] == E_ARG
    if records[0][2] == 1:                                                    # without a table any keyword id is its own token
        rc, need, a, b, c, f = _raw(b"abcdef", rec, DROP, 16)
        assert (rc, need) == (0, 1) and a[0] == 1


def test_every_other_argument_error():
    good = np.array([(2, 2, 0)], po.RECORD_DTYPE)                             # `bc` of abcdef
    assert _raw(b"abcdef", good, RUN, 16, [0, 3, 6])[:2] == (0, 3)
    assert _raw(b"abcdef", good, RUN, 16, [0, 2, 6])[0] == E_ARG              # the record crosses a text boundary
    assert _raw(b"abcdef", good, RUN, 16, [0, 1, 6])[:2] == (0, 3)            # (a boundary in front of it is none)
    assert _raw(b"abcdef", good, RUN, 16, [0, 3, 5, 6])[:2] == (0, 4)         # (one inside the run behind it cuts the run)
    assert _raw(b"abcdef", good, RUN, 16, [1, 3, 6])[0] == E_ARG              # offsets that do not begin with 0
    assert _raw(b"abcdef", good, RUN, 16, [0, 4, 3, 6])[0] == E_ARG           # that decrease
    assert _raw(b"abcdef", good, RUN, 16, [0, 3, 5])[0] == E_ARG              # that do not end with n_symbols
    assert _raw(b"abcdef", good, RUN, 16, [0, 6], n_texts=1 << 31)[0] == E_ARG
    assert _raw(b"abcdef", good, 3, 16)[0] == E_ARG                           # a mode above 2
    # SYMBOL: symbols of 1 or 2 bytes, gap_base <= 2^32 - 2^(8 x sym_bytes)
    assert _raw(b"abcdef", good, SYMBOL, 16, gap_base=(1 << 32) - 256)[:2] == (0, 5)
    assert _raw(b"abcdef", good, SYMBOL, 16, gap_base=(1 << 32) - 255)[0] == E_ARG
    assert _raw(b"abcdefgh", good, SYMBOL, 16, gap_base=(1 << 32) - 65536, sb=2)[:2] == (0, 3)
    assert _raw(b"abcdefgh", good, SYMBOL, 16, gap_base=(1 << 32) - 65535, sb=2)[0] == E_ARG
    assert _raw(b"abcdefghijkl", good, SYMBOL, 16, sb=4)[0] == E_ARG
    assert _raw(b"abcdefghijkl", good, RUN, 16, sb=4)[:2] == (0, 2)            # RUN and DROP take any symbol size
    assert _raw(b"abcdefghi", good, DROP, 16, sb=3)[:2] == (0, 1)
    L = acm.lib()
    n = C.c_uint64(0)
    f = np.zeros(4, np.uint64)
    assert L.acm_tokens_records(None, 6, 1, 0, None, 0, None, 0, None, 0, 0, RUN, None, None, None, 0, None, None) == E_ARG      # no n_tokens
    assert L.acm_tokens_records(None, 6, 0, 0, None, 0, None, 0, None, 0, 0, RUN, None, None, None, 0, C.byref(n), None) == E_ARG  # no symbol size
    assert L.acm_tokens_records(None, 6, 1, 0, None, 0, None, 0, None, 0, 0, RUN, None, None, None, 0, C.byref(n), f.ctypes.data) == E_ARG  # tok_first without offsets
    assert L.acm_tokens_records(None, 6, 1, 0, None, 0, None, 0, None, 0, 0, SYMBOL, None, None, None, 0, C.byref(n), None) == E_ARG   # SYMBOL reads the text
    assert L.acm_tokens_records(None, 6, 1, 0, None, 0, None, 0, None, 0, 0, RUN, None, None, None, 0, C.byref(n), None) == 0 and n.value == 1   # RUN does not


def _tokenize(h, text3, off, mode, cap, tok_of=None, nk=0, gap_base=0, ids=True):
    """acm_tokenize on a machine of 3-byte symbols: (rc, n_tokens, n_selected, ids, starts, lens, first)"""
    L = acm.lib()
    t = np.frombuffer(text3, np.uint8).copy() if len(text3) else np.zeros(3, np.uint8)
    o = np.asarray(off, np.uint64) if off is not None else None
    a = np.full(cap + 4, 0xA5A5A5A5, np.uint32)
    b = np.full(cap + 4, 0xA5A5A5A5, np.uint64)
    c = np.full(cap + 4, 0xA5A5A5A5, np.uint32)
    f = np.full((o.size if o is not None else 1), 0xA5A5A5A5, np.uint64)
    table = np.asarray(tok_of, np.uint32) if tok_of is not None else None
    need, m = C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    rc = L.acm_tokenize(h, t.ctypes.data, len(text3) // 3, o.ctypes.data if o is not None else None, o.size - 1 if o is not None else 0,
                        table.ctypes.data if table is not None else None, nk, gap_base, mode, a.ctypes.data if ids else None,
                        b.ctypes.data if ids else None, c.ctypes.data if ids else None, cap, C.byref(need), f.ctypes.data if o is not None else None,
                        C.byref(m))
    return rc, int(need.value), int(m.value), a, b, c, f


def test_acm_tokenize_on_the_host_loop():
    L = acm.lib()
    # (the second case has 6,000 matches: more than the record room the call begins with)
    for keywords, texts in ((KEYWORDS + [b"absent"], TEXTS + [b"qq", b"qq"]), (USHERS, [b"ushers" * 2000])):
        whole, off = b"".join(texts), offsets_of(texts)
        o = byte_oracle(keywords)
        tok_of = (np.arange(len(keywords), dtype=np.uint32) * 3 + 100)
        for offsets in (off, None):
            rec, sel = selection_of(o, whole, offsets)
            assert 0 < sel.size < rec.size
            for mode in (RUN, DROP):
                ids, starts, lens, first = tokens_by_definition(whole, sel, mode, 9, tok_of, offsets)
                n = ids.size
                h, keep = loop_machine(keywords)
                assert L.acm_scan_path(h) == 0
                rc, need, m, a, b, c, f = _tokenize(h, sym3(whole), offsets, mode, 0, tok_of, len(keywords), 9, ids=False)      # count
                assert (rc, need, m) == (0, n, sel.size) and L.acm_scan_path(h) == PATH_LOOP and _untouched(a, b, c)
                rc, need, m, a, b, c, f = _tokenize(h, sym3(whole), offsets, mode, n, tok_of, len(keywords), 9)                 # fill
                assert (rc, need, m) == (0, n, sel.size)
                assert np.array_equal(a[:n], ids) and np.array_equal(b[:n], starts) and np.array_equal(c[:n], lens) and _untouched(a[n:], b[n:], c[n:])
                if offsets is not None:
                    assert np.array_equal(f, first)
                # one token short: the need comes back, the path is recorded, tok_first is valid
                h2, keep2 = loop_machine(keywords)
                rc, need, m, a, b, c, f = _tokenize(h2, sym3(whole), offsets, mode, n - 1, tok_of, len(keywords), 9)
                assert (rc, need, m) == (E_OVERFLOW, n, sel.size) and L.acm_scan_path(h2) == PATH_LOOP and _untouched(a, b, c)
                if offsets is not None:
                    assert np.array_equal(f, first)
                L.acm_release(h2)
                # a table that is short of a keyword, whether it matched or not
                assert _tokenize(h, sym3(whole), offsets, mode, n, tok_of[:-1], len(keywords) - 1, 9)[0] == E_ARG
                # SYMBOL mode goes by the declared symbol size: 3 bytes have no byte fallback
                assert _tokenize(h, sym3(whole), offsets, SYMBOL, n, tok_of, len(keywords), 9)[0] == E_ARG
                L.acm_release(h)


def test_tokenize_arguments_are_checked_without_a_gpu():
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    t, a = np.zeros(3, np.uint8), np.zeros(16, np.uint32)
    bad_off = np.array([0, 2, 1], np.uint64)
    n, m = C.c_uint64(0), C.c_uint64(0)
    assert L.acm_tokenize(None, t.ctypes.data, 1, None, 0, None, 0, 0, RUN, a.ctypes.data, None, None, 4, C.byref(n), None, C.byref(m)) == E_ARG
    assert L.acm_tokenize(h, None, 1, None, 0, None, 0, 0, RUN, a.ctypes.data, None, None, 4, C.byref(n), None, C.byref(m)) == E_ARG
    assert L.acm_tokenize(h, t.ctypes.data, 1, None, 0, None, 0, 0, RUN, a.ctypes.data, None, None, 4, None, None, C.byref(m)) == E_ARG
    assert L.acm_tokenize(h, t.ctypes.data, 1, None, 0, None, 0, 0, 3, a.ctypes.data, None, None, 4, C.byref(n), None, C.byref(m)) == E_ARG
    assert L.acm_tokenize(h, t.ctypes.data, 1, bad_off.ctypes.data, 2, None, 0, 0, RUN, a.ctypes.data, None, None, 4, C.byref(n), None, C.byref(m)) == E_ARG
    assert L.acm_tokenize(h, t.ctypes.data, 1, None, 0, None, 0, 0, RUN, a.ctypes.data, None, None, 4, C.byref(n), bad_off.ctypes.data, C.byref(m)) == E_ARG
    assert L.acm_scan_path(h) == 0
    # the plan-level calls refuse a missing plan before they touch a device
    assert L.acm_gpu_tokens_records_device(None, None, 0, 0, None, 0, None, None, 0, None, 0, 0, RUN, None, None, None, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_tokens_device(None, None, 0, 0, None, 0, None, 0, None, None, 0, 0, RUN, None, None, None, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_tokens_host(None, t.ctypes.data, 1, None, 0, None, 0, 0, RUN, a.ctypes.data, None, None, 4, C.byref(n), None, C.byref(m)) == E_ARG
    assert L.acm_gpu_tokens_tmp_bytes(None, 16, 16) == 0 and L.acm_gpu_scan_tokens_tmp_bytes(None, 16, 16, 1) == 0
    L.acm_release(h)


def test_library_exports_the_token_symbols():
    L = acm.lib()
    for name in ("acm_tokens_records", "acm_gpu_tokens_tmp_bytes", "acm_gpu_tokens_records_device", "acm_gpu_scan_tokens_tmp_bytes",
                 "acm_gpu_scan_tokens_device", "acm_gpu_scan_tokens_host", "acm_tokenize"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
