"""Leftmost-longest selection without a GPU: acm_select_records (the sequential pass on the host) and
acm_select on a machine that takes the caller loop on the host (ACM_SCAN_PATH_CPU_LOOP).  The expected
answer is the definition of SELECT in plain Python over the ORACLE's records (tests/select_cases.py)."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, TEXTS
from tests.select_cases import assert_tiling, greedy, nontrivial, oracle_records, random_case
from tests.tally_cases import PATH_LOOP, byte_oracle, loop_machine, novel_words, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW


def _same(got, want):
    assert got.size == want.size and np.array_equal(got.astype(po.RECORD_DTYPE), want), (got[:8], want[:8])


def test_ushers_style_texts():
    o = byte_oracle([b"he", b"she", b"his", b"hers"])
    rec = oracle_records(o, b"ushers")
    assert rec.size == 3
    sel = binding.select_records(rec)
    assert [(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in sel] == [(3, 3, 1)]   # `she` alone
    _same(sel, greedy(rec))
    for keywords, text in (([b"he", b"she", b"his", b"hers"], b"To ushers: he found his pencil, but she could not find hers."),
                           (KEYWORDS, b"".join(TEXTS)),
                           ([b"a", b"aa", b"aaa", b"aaaa", b"ba", b"baa"], b"aaaabaaaabaab" * 40),
                           ([b"abcd", b"bc", b"cdxyz", b"d"], b"abcdxyz abcd bcdxyz" * 5)):
        rec = oracle_records(byte_oracle(keywords), text)
        want = greedy(rec)
        nontrivial(rec, want)
        got = binding.select_records(rec)
        _same(got, want)
        assert_tiling(got)


def test_the_novel_and_a_dictionary_of_its_own_words(novel_bytes):
    text = novel_bytes[:150000]
    rec = oracle_records(byte_oracle(novel_words(novel_bytes)), text)
    want = greedy(rec)
    nontrivial(rec, want)
    assert rec.size > 10000
    got = binding.select_records(rec)
    _same(got, want)
    assert_tiling(got)


def test_random_cases_and_the_smallest_sets():
    rng = np.random.default_rng(1975)
    some = 0
    for _ in range(200):
        keywords, text = random_case(rng, 8, 6, int(rng.integers(1, 301)))
        rec = oracle_records(byte_oracle(keywords), text)
        want = greedy(rec)
        got = binding.select_records(rec)
        _same(got, want)
        assert_tiling(got)
        some += 0 < want.size < rec.size
    assert some > 150
    assert binding.select_records(np.zeros(0, po.RECORD_DTYPE)).size == 0
    assert acm.lib().acm_select_records(None, 0) == 0
    one = np.array([(7, 3, 2)], po.RECORD_DTYPE)
    _same(binding.select_records(one), one)
    # the input array itself is selected in place in its front
    rec = oracle_records(byte_oracle([b"he", b"she", b"hers"]), b"ushers she")
    buf = rec.copy()
    n = acm.lib().acm_select_records(buf.ctypes.data, buf.size)
    _same(buf[:n], greedy(rec))


def _select(h, text3, capacity):
    L = acm.lib()
    t = np.frombuffer(text3, np.uint8).copy() if len(text3) else np.zeros(3, np.uint8)
    out = np.zeros(max(capacity, 1), po.RECORD_DTYPE)
    n = C.c_uint64(0xDEAD)
    rc = L.acm_select(h, t.ctypes.data, len(text3) // 3, out.ctypes.data, capacity, C.byref(n))
    return rc, int(n.value), out


def test_acm_select_on_the_host_loop(novel_bytes):
    L = acm.lib()
    for keywords, text in ((KEYWORDS + [b"absent"], b"".join(TEXTS)), (novel_words(novel_bytes), novel_bytes[:60000])):
        rec = oracle_records(byte_oracle(keywords), text)
        want = greedy(rec)
        nontrivial(rec, want)
        h, keep = loop_machine(keywords)
        assert L.acm_scan_path(h) == 0
        rc, n, out = _select(h, sym3(text), rec.size)
        assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
        _same(out[:n], want)
        # too little room for ALL matches: the count that suffices comes back, the repeat succeeds
        rc, n, out = _select(h, sym3(text), rec.size - 1)
        assert rc == E_OVERFLOW and n == rec.size
        rc, n, out = _select(h, sym3(text), n)
        assert rc == 0
        _same(out[:n], want)
        rc, n, out = _select(h, b"", 4)
        assert (rc, n) == (0, 0)
        L.acm_release(h)


def test_select_arguments_are_checked_without_a_gpu():
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    t = np.zeros(3, np.uint8)
    out = np.zeros(4, po.RECORD_DTYPE)
    n = C.c_uint64(0)
    assert L.acm_select(None, t.ctypes.data, 1, out.ctypes.data, 4, C.byref(n)) == E_ARG
    assert L.acm_select(h, None, 1, out.ctypes.data, 4, C.byref(n)) == E_ARG
    assert L.acm_select(h, t.ctypes.data, 1, None, 4, C.byref(n)) == E_ARG
    assert L.acm_select(h, t.ctypes.data, 1, out.ctypes.data, 4, None) == E_ARG
    assert L.acm_scan_path(h) == 0
    # the plan-level calls refuse a missing plan before they touch a device
    assert L.acm_gpu_select_records_device(None, None, 0, None, 0, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_select_device(None, None, 0, 0, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_select_host(None, t.ctypes.data, 1, 0, out.ctypes.data, 4, C.byref(n)) == E_ARG
    assert L.acm_gpu_select_tmp_bytes(None, 16, 16) == 0 and L.acm_gpu_scan_select_tmp_bytes(None, 16, 16) == 0
    assert L.acm_gpu_select_form(None) == E_ARG
    L.acm_release(h)


def test_library_exports_the_select_symbols():
    L = acm.lib()
    for name in ("acm_select_records", "acm_gpu_select_tmp_bytes", "acm_gpu_select_records_device", "acm_gpu_select_form",
                 "acm_gpu_scan_select_tmp_bytes", "acm_gpu_scan_select_device", "acm_gpu_scan_select_host", "acm_select"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
