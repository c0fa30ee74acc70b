"""acm_scan_from without a GPU: a machine whose symbols are 3 bytes wide takes the caller loop on the
host (ACM_SCAN_PATH_CPU_LOOP), continued from the caller's cursor.  A text is split into a prefix fed
symbol by symbol (acm_match), a middle fed in one acm_scan_from and a tail fed symbol by symbol
again, at EVERY pair of cut points -- inside "she|rs", inside the nested suffixes, at the ends.  The
expected records and the expected acm_match counts are the ORACLE's single loop over the whole text
(tests/flow_cases.py; the 3-byte letters map one to one to the oracle's bytes as in
tests/test_batch_cpu.py)."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.flow_cases import KEYWORDS, raw_machine3, split_scan, sym3

PATH_LOOP = 3
TEXT = b"ushers she sells hers; sshe"


def _oracle():
    o = po.Oracle(1, po.MEYER85)
    for kw in KEYWORDS:
        o.add_keyword(kw)
    return o


def test_scan_from_at_every_pair_of_cuts_equals_the_oracles_single_loop():
    h, keep = raw_machine3(KEYWORDS)
    L = acm.lib()
    want = _oracle().scan(TEXT)
    counts = np.bincount(want["end_pos"].astype(np.int64), minlength=len(TEXT))
    assert want.size > 15 and counts.max() == 2                       # "hers" ends "s" too; "she" ends "he"
    n = len(TEXT)
    cuts = [(a, b) for a in range(n + 1) for b in range(a, n + 1)]
    assert (4, 20) in cuts and (3, 4) in cuts                        # "ushe|rs", and a middle that is the "h" of "she" alone
    for a, b in cuts:
        split_scan(L, h, sym3(TEXT), 3, a, b, counts, want)
    assert L.acm_scan_path(h) == PATH_LOOP
    L.acm_release(h)


def test_a_keyword_cut_by_the_boundary_is_found_with_its_full_length():
    """ "ushe" then "rs": the middle's first record is "hers" (and "s") ending at its symbol 1, length 4 > 2"""
    h, keep = raw_machine3(KEYWORDS)
    L = acm.lib()
    first, second = np.frombuffer(sym3(b"ushe"), np.uint8).copy(), np.frombuffer(sym3(b"rs"), np.uint8).copy()
    cur = C.c_void_p(L.acm_initiate(h))
    rec = np.zeros(8, binding.RECORD_DTYPE)
    n = C.c_uint64(0)
    assert L.acm_scan_from(h, C.byref(cur), first.ctypes.data, 4, rec.ctypes.data, 8, C.byref(n)) == 0
    o = _oracle()
    assert np.array_equal(rec[:n.value], o.scan(b"ushe"))
    assert L.acm_scan_from(h, C.byref(cur), second.ctypes.data, 2, rec.ctypes.data, 8, C.byref(n)) == 0
    want = o.scan(b"ushers")
    want = want[want["end_pos"] >= 4].copy()
    want["end_pos"] -= np.uint64(4)
    assert n.value == want.size == 2 and np.array_equal(rec[:2], want) and rec[0]["length"] == 4 and rec[0]["end_pos"] == 1
    L.acm_release(h)


def test_scan_from_arguments_are_checked():
    h, keep = raw_machine3(KEYWORDS)
    other, keep2 = raw_machine3(KEYWORDS)
    L = acm.lib()
    t = np.frombuffer(sym3(b"she"), np.uint8).copy()
    rec = np.zeros(8, binding.RECORD_DTYPE)
    n = C.c_uint64(0)
    cur = C.c_void_p(L.acm_initiate(h))
    E = binding.ACM_GPU_E_ARG
    assert L.acm_scan_from(None, C.byref(cur), t.ctypes.data, 3, rec.ctypes.data, 8, C.byref(n)) == E
    assert L.acm_scan_from(h, None, t.ctypes.data, 3, rec.ctypes.data, 8, C.byref(n)) == E
    assert L.acm_scan_from(h, C.byref(C.c_void_p(None)), t.ctypes.data, 3, rec.ctypes.data, 8, C.byref(n)) == E
    assert L.acm_scan_from(other, C.byref(cur), t.ctypes.data, 3, rec.ctypes.data, 8, C.byref(n)) == E   # another machine's cursor
    assert L.acm_scan_from(h, C.byref(cur), None, 3, rec.ctypes.data, 8, C.byref(n)) == E
    assert L.acm_scan_from(h, C.byref(cur), t.ctypes.data, 3, None, 8, C.byref(n)) == E
    assert L.acm_scan_from(h, C.byref(cur), t.ctypes.data, 3, rec.ctypes.data, 8, None) == E
    assert cur.value == L.acm_initiate(h) and L.acm_scan_path(h) == 0
    # the flow calls check their handles before they touch a device
    assert L.acm_gpu_flows_create(None, 4, C.byref(C.c_void_p())) == E
    assert L.acm_gpu_scan_flows_tmp_bytes(None, None, 16, 16, 1) == 0
    assert L.acm_gpu_scan_flows_device(None, None, None, 0, None, None, 0, None, None, None, 0, None, None, 0, None) == E
    assert L.acm_gpu_scan_flows_host(None, None, None, 0, None, None, 0, None, None, None, 0, C.byref(n)) == E
    assert L.acm_gpu_flows_reset(None, None, 0, None) == E
    L.acm_release(h)
    L.acm_release(other)


def test_machine_scan_from_in_python():
    m = acm.Machine(3)
    for kw in KEYWORDS:
        buf = np.frombuffer(sym3(kw), np.uint8).copy()
        m._keep.append(buf)
        cur = C.c_void_p(m.L.acm_initiate(m.handle))
        for i in range(len(kw)):
            m.L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + 3 * i)
        m.L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    want = _oracle().scan(TEXT)
    cur, got, at = m.root(), [], 0
    for piece in (TEXT[:4], TEXT[4:5], b"", TEXT[5:19], TEXT[19:]):
        r, cur = m.scan_from(cur, sym3(piece))
        r = r.copy()
        r["end_pos"] += np.uint64(at)
        got.append(r)
        at += len(piece)
    assert m.scan_path == PATH_LOOP and np.array_equal(np.concatenate(got), want)
