"""Anchored matches and the dictionary lookup without a GPU: acm_anchored_records (the sequential pass
on the host, executed here as the definition's C form), acm_scan_anchored and acm_lookup on a machine
that takes the caller loop on the host (ACM_SCAN_PATH_CPU_LOOP), the argument errors.  The expected
answer is the definition of ANCHORED and LOOKUP in plain Python over the ORACLE's records
(tests/anchored_cases.py)."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests import anchored_cases as ac
from tests.batch_cases import oracle_batch
from tests.tally_cases import byte_oracle, loop_machine, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
PATH_LOOP = 3
NAMES = ("acm_anchored_records", "acm_gpu_scan_anchored_tmp_bytes", "acm_gpu_scan_anchored_device", "acm_gpu_lookup_tmp_bytes",
         "acm_gpu_lookup_device", "acm_gpu_scan_anchored_host", "acm_gpu_lookup_host", "acm_scan_anchored", "acm_lookup")


def _same(got, want):
    rec, tid, first = got
    assert rec.size == want[0].size and np.array_equal(rec.astype(po.RECORD_DTYPE), want[0]), (rec[:8], want[0][:8])
    assert np.array_equal(tid, want[1]) and np.array_equal(first, want[2])


def _call(records, offsets, mode, with_text_id=True, with_first=True):
    """acm_anchored_records through ctypes on a copy of `records`: (rc, n_kept, records, text_id, first) afterwards;
    text_id and first are pre-filled with a pattern"""
    a = np.array(records, dtype=po.RECORD_DTYPE, copy=True).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    tid = np.full(max(a.size, 1), 0xABABABAB, np.uint32)
    first = np.full(off.size, 0xCDCDCDCDCDCDCDCD, np.uint64)
    n = C.c_uint64(0xDEAD)
    rc = acm.lib().acm_anchored_records(off.ctypes.data, off.size - 1, mode, a.ctypes.data if a.size else None, a.size,
                                        tid.ctypes.data if with_text_id else None, first.ctypes.data if with_first else None, C.byref(n))
    return rc, int(n.value), a, tid, first


def test_hand_made_batch_in_all_three_modes():
    o = byte_oracle(ac.KEYWORDS)
    packed, off, want, look = ac.hand_made(o)
    rec, tid, first = oracle_batch(o, ac.TEXTS)
    for mode in ac.MODES:
        rc, n, a, t, f = _call(rec, off, mode)
        assert rc == 0
        _same((a[:n], t[:n], f), want[mode])
        assert np.all(t[n:] == 0xABABABAB)                       # nothing behind the kept records
        rc, n2, a2, t2, f2 = _call(rec, off, mode, with_text_id=False, with_first=False)
        assert rc == 0 and n2 == n and np.array_equal(a2[:n], a[:n]) and np.all(t2 == 0xABABABAB) and np.all(f2 == 0xCDCDCDCDCDCDCDCD)
        _same(binding.anchored_records(rec, off, mode), want[mode])
    _same(binding.anchored_records(rec, off, "whole"), want[ac.WHOLE])
    assert want[ac.PREFIXES][0].size == ac.N_PREFIXES == 29 and want[ac.LONGEST][0].size == 10 and want[ac.WHOLE][0].size == 8


def test_novel_words_batch_of_a_few_thousand_texts(novel_bytes):
    keywords, o, text, off, want, look = ac.novel_batch(novel_bytes)
    assert off.size - 1 >= 3000
    rec, t = ac.batch_records(o, text, off)
    for mode in ac.MODES:
        rc, n, a, tid, first = _call(rec, off, mode)
        assert rc == 0
        _same((a[:n], tid[:n], first), want[mode])
    # the raw records of the packed buffer are no batch's: some cross a cut
    raw = o.scan(text)
    assert raw.size > rec.size and _call(raw, off, ac.PREFIXES)[0] == E_ARG


def test_empty_batches_and_empty_texts():
    none = np.zeros(0, po.RECORD_DTYPE)
    rc, n, a, tid, first = _call(none, [0], ac.PREFIXES)
    assert (rc, n) == (0, 0) and first.tolist() == [0]
    rc, n, a, tid, first = _call(none, [0, 0, 0], ac.WHOLE)
    assert (rc, n) == (0, 0) and first.tolist() == [0, 0, 0]
    rc, n, a, tid, first = _call(none, [0, 4, 4, 9], ac.LONGEST)
    assert (rc, n) == (0, 0) and first.tolist() == [0, 0, 0, 0]


def test_every_argument_error_and_nothing_modified():
    o = byte_oracle(ac.KEYWORDS)
    packed, off, want, look = ac.hand_made(o)
    rec, tid, first = oracle_batch(o, ac.TEXTS)
    n_sym = int(off[-1])

    def refused(records=rec, offsets=off, mode=ac.PREFIXES):
        rc, n, a, t, f = _call(records, offsets, mode)
        assert rc == E_ARG and np.array_equal(a, np.asarray(records, po.RECORD_DTYPE)) and np.all(t == 0xABABABAB) and np.all(f == 0xCDCDCDCDCDCDCDCD)

    refused(mode=0)
    refused(mode=4)
    bad = off.copy()
    bad[0] = 1
    refused(offsets=bad)
    bad = off.copy()
    bad[5], bad[6] = off[6], off[5]                              # a decrease
    assert bad[5] > bad[6]
    refused(offsets=bad)
    refused(offsets=off[:-1])                                    # the last record lies outside [0, offsets[n_texts])
    b = rec.copy()
    b["end_pos"][-1] = n_sym
    refused(records=b)
    b = rec.copy()
    b["length"][2] = 0
    refused(records=b)
    b = rec.copy()
    b["length"][0] = int(b["end_pos"][0]) + 2                    # a start below the buffer
    refused(records=b)
    cross = np.zeros(1, po.RECORD_DTYPE)                         # "he" | "rs": `her` across the cut
    cross[0] = (int(off[13]), 3, 2)
    refused(records=cross)
    L = acm.lib()
    a = rec.copy()
    n = C.c_uint64(0)
    assert L.acm_anchored_records(None, off.size - 1, 1, a.ctypes.data, a.size, None, None, C.byref(n)) == E_ARG
    assert L.acm_anchored_records(off.ctypes.data, off.size - 1, 1, None, a.size, None, None, C.byref(n)) == E_ARG
    assert L.acm_anchored_records(off.ctypes.data, off.size - 1, 1, a.ctypes.data, a.size, None, None, None) == E_ARG
    assert np.array_equal(a, rec)
    # the plan-level calls refuse a missing plan before they touch a device
    assert L.acm_gpu_scan_anchored_tmp_bytes(None, 4) == 0 and L.acm_gpu_lookup_tmp_bytes(None, 4) == 0
    assert L.acm_gpu_scan_anchored_device(None, None, 0, None, 0, 1, None, None, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_lookup_device(None, None, 0, None, 0, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_anchored_host(None, None, off.ctypes.data, 0, 1, None, None, None, 0, C.byref(n)) == E_ARG
    assert L.acm_gpu_lookup_host(None, None, off.ctypes.data, 0, a.ctypes.data, None, None) == E_ARG
    assert L.acm_scan_anchored(None, None, off.ctypes.data, 0, 1, None, None, None, 0, C.byref(n)) == E_ARG
    assert L.acm_lookup(None, None, off.ctypes.data, 0, a.ctypes.data, None, None) == E_ARG


def _machine_anchored(h, text3, off, mode, capacity, with_sides=True):
    out = np.zeros(max(capacity, 1), po.RECORD_DTYPE)
    tid = np.full(max(capacity, 1), 0xABABABAB, np.uint32)
    first = np.full(off.size, 0xCDCDCDCDCDCDCDCD, np.uint64)
    n = C.c_uint64(0xDEAD)
    rc = acm.lib().acm_scan_anchored(h, text3.ctypes.data, off.ctypes.data, off.size - 1, mode, out.ctypes.data,
                                     tid.ctypes.data if with_sides else None, first.ctypes.data if with_sides else None, capacity, C.byref(n))
    return rc, int(n.value), out, tid, first


def _machine_lookup(h, text3, off, which=(True, True, True)):
    res = [np.full(off.size - 1, 0x5A5A5A5A, np.uint32) for _ in range(3)]
    rc = acm.lib().acm_lookup(h, text3.ctypes.data, off.ctypes.data, off.size - 1, *[r.ctypes.data if w else None for r, w in zip(res, which)])
    return rc, res


def test_acm_scan_anchored_and_acm_lookup_on_the_host_loop():
    L = acm.lib()
    # the hand-made batch first: 3-byte symbols, the caller loop on the host
    o = byte_oracle(ac.KEYWORDS)
    packed, off, want, look = ac.hand_made(o)
    h, keep = loop_machine(ac.KEYWORDS)
    t3 = np.frombuffer(sym3(packed), np.uint8).copy()
    assert L.acm_scan_path(h) == 0
    for mode in ac.MODES:
        rc, n, out, tid, first = _machine_anchored(h, t3, off, mode, 29)
        assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
        _same((out[:n], tid[:n], first), want[mode])
        assert np.all(tid[n:] == 0xABABABAB)
        rc, n, out, tid, first = _machine_anchored(h, t3, off, mode, 29, with_sides=False)
        assert rc == 0 and np.array_equal(out[:n], want[mode][0])
    # room for the anchored records only: one less overflows with the need, and first[] is complete
    rc, n, out, tid, first = _machine_anchored(h, t3, off, ac.PREFIXES, 28)
    assert rc == E_OVERFLOW and n == 29 and np.array_equal(first, want[ac.PREFIXES][2]) and np.all(tid == 0xABABABAB)
    for mode in (ac.LONGEST, ac.WHOLE):                          # capacity = n_texts cannot overflow
        assert _machine_anchored(h, t3, off, mode, off.size - 1)[0] == 0
    rc, res = _machine_lookup(h, t3, off)
    assert rc == 0 and all(np.array_equal(g, w) for g, w in zip(res, look))
    rc, res = _machine_lookup(h, t3, off, which=(False, True, False))
    assert rc == 0 and np.array_equal(res[1], look[1]) and np.all(res[0] == 0x5A5A5A5A) and np.all(res[2] == 0x5A5A5A5A)
    assert _machine_lookup(h, t3, off, which=(False, False, False))[0] == E_ARG
    assert _machine_anchored(h, t3, off, 0, 29)[0] == E_ARG and _machine_anchored(h, t3, off, 4, 29)[0] == E_ARG
    bad = off.copy()
    bad[3] = bad[4] + 1
    assert _machine_anchored(h, t3, bad, ac.PREFIXES, 29)[0] == E_ARG and _machine_lookup(h, t3, bad)[0] == E_ARG
    # too many texts for the prefix sum's 31-bit count of n_texts + 1 items: refused before an offset is looked at
    nf = C.c_uint64(0)
    assert L.acm_scan_anchored(h, t3.ctypes.data, off.ctypes.data, (1 << 31) - 1, ac.PREFIXES, None, None, None, 0, C.byref(nf)) == E_ARG
    empty = np.zeros(1, np.uint64)
    rc, n, out, tid, first = _machine_anchored(h, t3, empty, ac.PREFIXES, 4)
    assert (rc, n) == (0, 0) and first.tolist() == [0]
    L.acm_release(h)


def test_machine_calls_on_a_novel_words_batch(novel_bytes):
    L = acm.lib()
    part = novel_bytes[:150000]
    from tests.tally_cases import novel_words
    keywords = novel_words(novel_bytes)
    o = byte_oracle(keywords)
    off, chosen = ac.make_cuts(len(part), o.scan(part), n_chosen=1200, n_random=1200)
    want, look = ac.expected(o, part, off)
    with_prefix, with_whole, none, nested = ac.nontrivial(want, look, chosen, many=False)
    assert with_prefix >= 1000 and with_whole >= 400 and none >= 400 and nested >= 30
    h, keep = loop_machine(keywords)
    t3 = np.frombuffer(sym3(part), np.uint8).copy()
    for mode in ac.MODES:
        rc, n, out, tid, first = _machine_anchored(h, t3, off, mode, want[ac.PREFIXES][0].size)
        assert rc == 0
        _same((out[:n], tid[:n], first), want[mode])
    rc, res = _machine_lookup(h, t3, off)
    assert rc == 0 and all(np.array_equal(g, w) for g, w in zip(res, look))
    assert L.acm_scan_path(h) == PATH_LOOP
    L.acm_release(h)


def test_library_exports_the_anchored_symbols():
    L = acm.lib()
    for name in NAMES:
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
    assert (acm.ACM_ANCHORED_PREFIXES, acm.ACM_ANCHORED_LONGEST, acm.ACM_ANCHORED_WHOLE) == ac.MODES and acm.ACM_LOOKUP_NONE == ac.NONE


def test_header_section_declares_the_anchored_functions():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "acm_gpu.h")) as f:
        header = f.read()
    section = header[header.index("anchored matches and dictionary lookup"):header.index("streaming scan")]
    declared = set(re.findall(r"^(?:int|size_t) (acm_\w+) \(", section, re.M))
    assert declared == set(NAMES), declared ^ set(NAMES)
    for mode in ("ACM_ANCHORED_PREFIXES 1", "ACM_ANCHORED_LONGEST 2", "ACM_ANCHORED_WHOLE 3", "ACM_LOOKUP_NONE 0xFFFFFFFFu"):
        assert "#define " + mode in section
