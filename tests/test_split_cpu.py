"""A buffer cut into texts without a GPU: acm_split_offsets (the sequential pass) and acm_grep_lines on a
machine with a comparator of its own over 3-byte symbols, which takes the caller loop on the host
(ACM_SCAN_PATH_CPU_LOOP).  Expected offsets always come from numpy (tests/split_cases.py), expected hits
from the ORACLE's scan of every text alone (tests/grep_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import KEYWORDS
from tests.grep_cases import GREP_TEXTS, check, expected, nontrivial, oracle_hits
from tests.split_cases import DELIM1, DELIM16, EDGES, expected_offsets, expected_raw, straddle, wide, with_delims
from tests.tally_cases import PATH_LOOP, byte_oracle, loop_machine, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.mark.parametrize("sb", [1, 2, 4, 8, 3])
@pytest.mark.parametrize("runs", [False, True])
@pytest.mark.parametrize("delims", [DELIM1, DELIM16], ids=["one", "sixteen"])
def test_split_offsets_on_the_edges(sb, runs, delims):
    for text in EDGES:
        t = with_delims(text, delims)
        raw, draw = wide(t, sb), wide(delims, sb)
        want = expected_raw(raw, draw, sb, runs)
        assert want[0] == 0 and want[-1] == len(t) and np.all(np.diff(want.astype(np.int64)) > 0)
        got = binding.split_offsets(raw, draw, runs=runs, sym_size=sb)
        assert np.array_equal(got, want), (text, got, want)
    # the header's example
    if delims == DELIM1:
        assert binding.split_offsets(wide(b"a\n\nb", sb), wide(b"\n", sb), runs=False, sym_size=sb).tolist() == [0, 2, 3, 4]
        assert binding.split_offsets(wide(b"a\n\nb", sb), wide(b"\n", sb), runs=True, sym_size=sb).tolist() == [0, 3, 4]
        assert binding.split_offsets(wide(b"\n\na", sb), wide(b"\n", sb), runs=True, sym_size=sb).tolist() == [0, 2, 3]


@pytest.mark.parametrize("sb", [1, 2, 4, 8, 3])
@pytest.mark.parametrize("runs", [False, True])
def test_split_offsets_count_only_and_capacity(sb, runs):
    L = acm.lib()
    t = b"\n\none two\n\nthree\nfour"
    raw, draw = wide(t, sb), wide(b"\n", sb)
    want = expected_raw(raw, draw, sb, runs)
    need = want.size - 1
    assert need == (4 if runs else 6)
    n = C.c_uint64(99)
    # count only: no offsets, the capacity is ignored
    assert L.acm_split_offsets(raw.ctypes.data, len(t), sb, draw.ctypes.data, 1, int(runs), None, 0, C.byref(n)) == 0 and n.value == need
    # one too little room: the count, nothing written
    buf = np.full(need + 3, GUARD, np.uint64)
    n.value = 99
    assert L.acm_split_offsets(raw.ctypes.data, len(t), sb, draw.ctypes.data, 1, int(runs), buf[1:].ctypes.data, need - 1, C.byref(n)) == E_OVERFLOW
    assert n.value == need and np.all(buf == GUARD)
    # exactly enough: nothing written beside offsets[0 .. need]
    assert L.acm_split_offsets(raw.ctypes.data, len(t), sb, draw.ctypes.data, 1, int(runs), buf[1:].ctypes.data, need, C.byref(n)) == 0
    assert n.value == need and np.array_equal(buf[1:need + 2], want) and buf[0] == GUARD and buf[need + 2] == GUARD


def test_split_offsets_arguments():
    L = acm.lib()
    text = np.frombuffer(b"ab\ncd", np.uint8)
    d = np.frombuffer(DELIM16 + b"#", np.uint8)
    n = C.c_uint64(0)

    def call(n_delims=1, flags=0, sb=1, delims=d.ctypes.data, n_texts=C.byref(n), t=text.ctypes.data):
        return L.acm_split_offsets(t, text.size, sb, delims, n_delims, flags, None, 0, n_texts)
    assert call() == 0 and n.value == 2
    assert call(n_delims=16) == 0
    assert call(n_delims=0) == E_ARG and call(n_delims=17) == E_ARG and call(flags=2) == E_ARG
    assert call(sb=0) == E_ARG and call(delims=None) == E_ARG and call(n_texts=None) == E_ARG and call(t=None) == E_ARG
    # no text at all
    assert L.acm_split_offsets(None, 0, 1, d.ctypes.data, 1, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    off = np.full(1, GUARD, np.uint64)
    assert L.acm_split_offsets(None, 0, 1, d.ctypes.data, 1, 1, off.ctypes.data, 0, C.byref(n)) == 0 and n.value == 0 and off[0] == 0


@pytest.mark.parametrize("sb", [2, 4, 8])
@pytest.mark.parametrize("runs", [False, True])
def test_delimiter_bytes_across_two_symbols_are_no_delimiter(sb, runs):
    text, delim = straddle(sb)
    assert expected_offsets(text, delim, runs).tolist() == [0, 3]
    assert binding.split_offsets(text, delim, runs=runs).tolist() == [0, 3]                    # ONE cut
    longer = np.concatenate([text, text[:2], np.array([0x41], text.dtype)])
    assert binding.split_offsets(longer, delim, runs=runs).tolist() == [0, 3, 6]


def _lines_case():
    """GREP_TEXTS joined with a newline; the delimiters are the newline and "r", which cuts "he|r|s" (a
    match of the whole buffer that no text holds)"""
    o = byte_oracle(KEYWORDS)
    text = np.frombuffer(b"\n".join(GREP_TEXTS), np.uint8)
    delims = b"\nr"
    return o, text, delims


@pytest.mark.parametrize("runs", [False, True])
@pytest.mark.parametrize("invert", [False, True])
def test_grep_lines_on_the_host_loop(runs, invert):
    o, text, delims = _lines_case()
    off = expected_offsets(text, np.frombuffer(delims, np.uint8), runs)
    hits = oracle_hits(o, text, off)
    nontrivial(o, text, off, hits)
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    raw = np.frombuffer(sym3(bytes(text)), np.uint8).copy()
    draw = np.frombuffer(sym3(delims), np.uint8).copy()
    want = expected(raw, off, hits, invert, sym_size=3)
    n, n_sym = off.size - 1, text.size

    def call(texts_capacity, out_capacity, per_text=True):
        got_off, out_off = np.full(texts_capacity + 2, GUARD, np.uint64), np.full(texts_capacity + 2, GUARD, np.uint64)
        got_hits, kept = np.full(texts_capacity + 1, GUARD, np.uint64), np.full(texts_capacity + 1, 0xA5A5A5A5, np.uint32)
        out = np.full(out_capacity * 3 + 3, 0xA5, np.uint8)
        nt, nk, total, sym = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
        rc = L.acm_grep_lines(h, raw.ctypes.data, n_sym, draw.ctypes.data, len(delims), int(runs), int(invert), C.byref(nt), C.byref(nk), C.byref(total),
                              out.ctypes.data, out_capacity, C.byref(sym), texts_capacity, *((got_off.ctypes.data, got_hits.ctypes.data, kept.ctypes.data,
                                                                                             out_off.ctypes.data) if per_text else (None,) * 4))
        return rc, nt.value, nk.value, total.value, sym.value, got_off, got_hits, kept, out_off, out
    assert L.acm_scan_path(h) == 0
    rc, nt, nk, total, sym, got_off, got_hits, kept, out_off, out = call(n, n_sym)
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP and nt == n
    assert np.array_equal(got_off[:n + 1], off) and got_off[n + 1] == GUARD
    got = binding.Grepped(got_hits[:n], kept[:nk], int(nk), int(total), None, out[:sym * 3], out_off[:nk + 1], int(sym))
    check(got, hits, want, 3, "acm_grep_lines")
    assert got_hits[n] == GUARD and kept[nk] == 0xA5A5A5A5 and out_off[nk + 1] == GUARD and np.all(out[sym * 3:] == 0xA5)
    # the binding: the same through Machine-level plumbing is covered on the GPU; here no per-text array at all
    rc, nt, nk2, total2, sym2 = call(0, n_sym, per_text=False)[:5]
    assert rc == 0 and (nt, nk2, total2, sym2) == (n, nk, total, sym)
    # the room for texts one too small: its own overflow, only n_texts is valid, nothing written
    rc, nt, _, _, _, got_off, got_hits, kept, out_off, out = call(n - 1, n_sym)
    assert rc == E_OVERFLOW and nt == n
    assert np.all(got_off == GUARD) and np.all(got_hits == GUARD) and np.all(kept == 0xA5A5A5A5) and np.all(out_off == GUARD) and np.all(out == 0xA5)
    # the room of the output one too small: the other overflow, everything but `out` is valid
    need = int(want[1][-1])
    assert need > 0
    rc, nt, nk3, total3, sym3_, got_off, got_hits, kept, out_off, out = call(n, need - 1)
    assert rc == E_OVERFLOW and nt == n and sym3_ == need and np.all(out == 0xA5)
    got = binding.Grepped(got_hits[:n], kept[:nk3], int(nk3), int(total3), None, None, out_off[:nk3 + 1], int(sym3_))
    check(got, hits, want, 3, "one symbol short")
    assert np.array_equal(got_off[:n + 1], off)
    L.acm_release(h)


def test_grep_lines_arguments_and_exports():
    L = acm.lib()
    for name in ("acm_split_offsets", "acm_gpu_split_tmp_bytes", "acm_gpu_split_device", "acm_gpu_split_host", "acm_gpu_grep_lines_host",
                 "acm_grep_lines"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
    h, keep = loop_machine(KEYWORDS)
    raw = np.frombuffer(sym3(b"us\nhers\n"), np.uint8).copy()
    d = np.frombuffer(sym3(b"\n" * 17), np.uint8).copy()
    nt, nk = C.c_uint64(0), C.c_uint64(0)

    def call(machine=h, n_delims=1, sflags=0, gflags=0, n_texts=C.byref(nt), n_kept=C.byref(nk), delims=d.ctypes.data):
        return L.acm_grep_lines(machine, raw.ctypes.data, 8, delims, n_delims, sflags, gflags, n_texts, n_kept, None, None, 0, None, 0, None, None,
                                None, None)
    assert call() == 0 and (nt.value, nk.value) == (2, 2)
    assert call(gflags=1) == 0 and (nt.value, nk.value) == (2, 0)
    for bad in (dict(machine=None), dict(n_delims=0), dict(n_delims=17), dict(sflags=2), dict(gflags=2), dict(n_texts=None), dict(n_kept=None),
                dict(delims=None)):
        assert call(**bad) == E_ARG, bad
    L.acm_release(h)
    # the plan-level calls refuse before they touch a device
    n = C.c_uint64(0)
    assert L.acm_gpu_split_tmp_bytes(None, 16) == 0
    assert L.acm_gpu_split_device(None, None, 0, d.ctypes.data, 1, 0, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_split_host(None, None, 0, d.ctypes.data, 1, 0, None, 0, C.byref(n)) == E_ARG
    assert L.acm_gpu_grep_lines_host(None, None, 0, d.ctypes.data, 1, 0, 0, C.byref(nt), C.byref(nk), None, None, 0, None, 0, None, None, None,
                                     None) == E_ARG
