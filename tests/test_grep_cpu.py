"""grep over a batch without a GPU: acm_grep_gather (the sequential pass) and acm_grep on a machine
with a comparator of its own over 3-byte symbols, which takes the caller loop on the host
(ACM_SCAN_PATH_CPU_LOOP).  The expected answer is always derived from the ORACLE's scan of every text
alone (tests/grep_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import KEYWORDS, offsets_of
from tests.grep_cases import GREP_TEXTS, check, expected, nontrivial, oracle_hits
from tests.tally_cases import PATH_LOOP, byte_oracle, loop_machine, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD = 0xA5


def _wide(text, sb):
    """bytes -> raw bytes of symbols of sb bytes: the letter c is (c, c ^ 0x5A, 7, 8, ...)[:sb]"""
    w = np.frombuffer(bytes(text), np.uint8)
    cols = [w, w ^ 0x5A] + [np.full_like(w, 7 + k) for k in range(6)]
    return np.stack(cols[:sb], axis=1).reshape(-1).copy()


def _case():
    o = byte_oracle(KEYWORDS)
    text = np.frombuffer(b"".join(GREP_TEXTS), np.uint8)
    off = offsets_of(GREP_TEXTS)
    hits = oracle_hits(o, text, off)
    nontrivial(o, text, off, hits)
    return o, text, off, hits


@pytest.mark.parametrize("sb", [1, 2, 4, 8, 3])
@pytest.mark.parametrize("invert", [False, True])
def test_gather_on_the_boundary_cases(sb, invert):
    o, text, off, hits = _case()
    raw = _wide(text, sb)
    want = expected(raw, off, hits, invert, sym_size=sb)
    assert want[0].size and want[2].size                                           # both flags keep a text that is not empty
    got = binding.grep_gather(raw, off, hits, invert=invert, sym_size=sb)
    check(got, hits, want, sb, "gather")
    got = binding.grep_gather(raw, off, hits, invert=invert, sym_size=sb, gather=False)
    assert got.out is None
    check(got, hits, want, sb, "no gather")
    # one symbol too little room: the need, `out` untouched, kept and out_offsets valid
    L = acm.lib()
    need = int(want[1][-1])
    out = np.full((need - 1) * sb, GUARD, np.uint8)
    kept = np.full(off.size - 1, 0xFFFFFFFF, np.uint32)
    out_off = np.full(off.size, 0xFFFFFFFFFFFFFFFF, np.uint64)
    nk, sym = C.c_uint64(99), C.c_uint64(99)
    rc = L.acm_grep_gather(raw.ctypes.data, sb, off.ctypes.data, off.size - 1, hits.ctypes.data, int(invert), kept.ctypes.data, C.byref(nk),
                           out.ctypes.data, need - 1, out_off.ctypes.data, C.byref(sym))
    assert rc == E_OVERFLOW and sym.value == need and np.all(out == GUARD)
    assert nk.value == want[0].size and np.array_equal(kept[:nk.value], want[0]) and np.array_equal(out_off[:nk.value + 1], want[1])
    assert np.all(kept[nk.value:] == 0xFFFFFFFF) and np.all(out_off[nk.value + 1:] == 0xFFFFFFFFFFFFFFFF)


def test_gather_arguments():
    L = acm.lib()
    o, text, off, hits = _case()
    nk, sym = C.c_uint64(99), C.c_uint64(99)

    def call(offsets=off, n_texts=None, flags=0, h=hits, sb=1, n_kept=C.byref(nk)):
        n = offsets.size - 1 if n_texts is None else n_texts
        return L.acm_grep_gather(text.ctypes.data, sb, offsets.ctypes.data if offsets is not None else None, n,
                                 h.ctypes.data if h is not None else None, flags, None, n_kept, None, 0, None, C.byref(sym))
    assert call() == 0 and nk.value == np.count_nonzero(hits) and sym.value == int((np.diff(off.astype(np.int64)))[hits > 0].sum())
    # no text at all: nothing kept, an empty output
    assert call(offsets=np.zeros(1, np.uint64), h=None) == 0 and nk.value == 0 and sym.value == 0
    out_off = np.full(1, 77, np.uint64)
    assert L.acm_grep_gather(None, 1, np.zeros(1, np.uint64).ctypes.data, 0, None, 1, None, C.byref(nk), None, 0, out_off.ctypes.data, None) == 0
    assert nk.value == 0 and out_off[0] == 0
    # offsets that break the contract
    bad = off.copy()
    bad[3], bad[4] = off[4] + 1, off[3]
    assert bad[3] > bad[4] and call(offsets=bad) == E_ARG
    first = off.copy()
    first[0] = 1
    assert call(offsets=first) == E_ARG
    assert call(offsets=None, n_texts=3) == E_ARG and call(flags=2) == E_ARG and call(sb=0) == E_ARG and call(h=None) == E_ARG
    assert call(n_kept=None) == E_ARG and call(n_texts=1 << 31) == E_ARG


@pytest.mark.parametrize("invert", [False, True])
def test_grep_on_the_host_loop(invert):
    """3-byte symbols: no GPU path takes the machine.  "us|hers" and "sh|e" cut a keyword by a text boundary"""
    o, text, off, hits = _case()
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    assert L.acm_scan_path(h) == 0
    raw = np.frombuffer(sym3(bytes(text)), np.uint8).copy()
    want = expected(raw, off, hits, invert, sym_size=3)
    n = off.size - 1
    got_hits, kept, out_off = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
    out = np.full(int(off[-1]) * 3, GUARD, np.uint8)
    nk, total, sym = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
    rc = L.acm_grep(h, raw.ctypes.data, off.ctypes.data, n, int(invert), got_hits.ctypes.data, kept.ctypes.data, C.byref(nk), C.byref(total),
                    out.ctypes.data, int(off[-1]), out_off.ctypes.data, C.byref(sym))
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    got = binding.Grepped(got_hits, kept[:nk.value], int(nk.value), int(total.value), None, out[:sym.value * 3], out_off[:nk.value + 1],
                          int(sym.value))
    check(got, hits, want, 3, "acm_grep")
    assert np.all(out[sym.value * 3:] == GUARD)
    # every output but n_kept is optional
    nk2 = C.c_uint64(99)
    assert L.acm_grep(h, raw.ctypes.data, off.ctypes.data, n, int(invert), None, None, C.byref(nk2), None, None, 0, None, None) == 0
    assert nk2.value == nk.value
    # an output with one symbol too little room: the need, kept still right
    small = np.full((sym.value - 1) * 3, GUARD, np.uint8)
    kept[:] = 0
    rc = L.acm_grep(h, raw.ctypes.data, off.ctypes.data, n, int(invert), None, kept.ctypes.data, C.byref(nk2), None, small.ctypes.data,
                    sym.value - 1, None, C.byref(sym))
    assert rc == E_OVERFLOW and sym.value == int(want[1][-1]) and np.all(small == GUARD) and np.array_equal(kept[:nk2.value], want[0])
    # arguments: no machine, no n_kept, offsets that decrease, flags
    bad = off.copy()
    bad[3], bad[4] = off[4] + 1, off[3]
    for args in ((None, off, 0, C.byref(nk2)), (h, off, 0, None), (h, bad, 0, C.byref(nk2)), (h, off, 2, C.byref(nk2))):
        assert L.acm_grep(args[0], raw.ctypes.data, args[1].ctypes.data, n, args[2], None, None, args[3], None, None, 0, None, None) == E_ARG
    L.acm_release(h)


def test_plan_level_calls_refuse_before_they_touch_a_device():
    L = acm.lib()
    nk = C.c_uint64(0)
    off = np.zeros(1, np.uint64)
    assert L.acm_gpu_grep_tmp_bytes(None, 16, 16, 0, 0) == 0
    assert L.acm_gpu_grep_host(None, None, off.ctypes.data, 0, 0, None, None, C.byref(nk), None, None, 0, None, None) == E_ARG
    assert L.acm_gpu_grep_device(None, None, 0, None, 0, 0, 16, 16, None, None, None, None, None, None, 0, None, None, None, 0, None) == E_ARG


def test_library_exports_the_grep_symbols():
    L = acm.lib()
    for name in ("acm_grep_gather", "acm_gpu_grep_tmp_bytes", "acm_gpu_grep_device", "acm_gpu_grep_host", "acm_grep"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
