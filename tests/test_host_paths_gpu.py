"""What the host-buffer entry points share (csrc/acm_gpu.hip: DeviceTemps, download_records, routed_scan):
a call that fails for want of room leaves nothing behind that disturbs the next call on the same plan.
One tiny known answer -- the README's he, she, his, hers on "ushers" x 64 -- through every entry point in
turn: first with too little room (ACM_GPU_E_OVERFLOW and the capacity that suffices), then with room
(exactly the ORACLE's answer), then the plan's status.  The expected records are the oracle's, never the
library's own."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import oracle_batch
from tests.cases import build_pair
from tests.select_cases import assert_tiling, greedy

pytestmark = pytest.mark.gpu

KEYWORDS = [b"he", b"she", b"his", b"hers"]
TEXT = np.frombuffer(b"ushers" * 64, np.uint8)                # 384 symbols
CUTS = [0, 100, 100, TEXT.size]                              # "ushe|rs": a keyword across the cut, then an empty text
OVERFLOW = binding.ACM_GPU_E_OVERFLOW


@pytest.fixture(scope="module")
def case():
    """(machine, plan, the oracle's records of TEXT, its batch answer for CUTS, its selection), with the
    preconditions shown from the oracle alone"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    m, o = build_pair(KEYWORDS, 1)
    rec = o.scan(TEXT)
    assert rec.size > 2, "capacity 2 must overflow"
    sel = greedy(rec)
    assert 0 < sel.size < rec.size, "the selection must leave records out"
    assert_tiling(sel)
    batch = oracle_batch(o, [TEXT[CUTS[t]:CUTS[t + 1]] for t in range(3)])
    assert 0 < batch[0].size < rec.size
    for a in (rec, sel) + tuple(batch):
        a.setflags(write=False)
    return m, m.plan(0), rec, batch, sel


def _same(got, want):
    assert got.size == want.size and np.array_equal(got.astype(po.RECORD_DTYPE), want), (got.size, want.size, got[:4], want[:4])


def _same_batch(got, want):
    for g, w, name in zip(got, want, ("records", "text_id", "first")):
        assert g.shape == w.shape and np.array_equal(g, w), (name, g.shape, w.shape)


def _room(cap):
    return np.zeros(cap, po.RECORD_DTYPE), C.c_uint64(0)


def test_plan_scan_host(case):
    m, plan, rec, batch, sel = case
    out, n = _room(2)
    rc = acm.lib().acm_gpu_scan_host(plan.h, TEXT.ctypes.data, TEXT.size, 0, 0, out.ctypes.data, 2, C.byref(n))
    assert rc == OVERFLOW and n.value == rec.size
    _same(plan.scan_host(TEXT, capacity=rec.size), rec)
    plan.status()


def test_plan_scan_batch_host(case):
    m, plan, rec, batch, sel = case
    off = np.array(CUTS, np.uint64)
    out, n = _room(2)
    rc = acm.lib().acm_gpu_scan_batch_host(plan.h, TEXT.ctypes.data, off.ctypes.data, 3, out.ctypes.data, None, None, 2, C.byref(n))
    assert rc == OVERFLOW and n.value == rec.size             # (the concatenation's records are found first)
    _same_batch(plan.scan_batch_host(TEXT, off, capacity=rec.size), batch)
    plan.status()


def test_flows_scan_host(case):
    m, plan, rec, batch, sel = case
    off = np.array(CUTS, np.uint64)
    flows = plan.flows(3)                                    # fresh: every text begins at the root, text t is flow t
    out, n = _room(2)
    rc = acm.lib().acm_gpu_scan_flows_host(plan.h, flows.h, TEXT.ctypes.data, TEXT.size, off.ctypes.data, None, 3, out.ctypes.data, None, None, 2,
                                           C.byref(n))
    assert rc == OVERFLOW and n.value == rec.size
    _same_batch(flows.scan_host(TEXT, off, capacity=rec.size), batch)
    plan.status()
    flows.close()


def test_plan_scan_select_host(case):
    m, plan, rec, batch, sel = case
    out, n = _room(1)
    rc = acm.lib().acm_gpu_scan_select_host(plan.h, TEXT.ctypes.data, TEXT.size, 0, out.ctypes.data, 1, C.byref(n))
    assert rc == OVERFLOW and n.value == rec.size             # (all matches are found first)
    _same(plan.scan_select_host(TEXT, capacity=rec.size), sel)
    plan.status()


def test_plan_tally_host(case, monkeypatch):
    m, plan, rec, batch, sel = case
    want = np.bincount(rec["keyword_id"].astype(np.int64), minlength=len(KEYWORDS)).astype(np.uint64)
    monkeypatch.setenv("ACM_GPU_TALLY_CAPACITY", "2")        # the first attempt overflows, the second cannot
    tally, total = plan.tally_host(TEXT)
    assert total == rec.size and np.array_equal(tally, want), (total, tally, want)
    monkeypatch.delenv("ACM_GPU_TALLY_CAPACITY")
    tally, total = plan.tally_host(TEXT)
    assert total == rec.size and np.array_equal(tally, want), (total, tally, want)
    plan.status()


def test_machine_level_calls(case, monkeypatch):
    """the same two steps through acm_scan, acm_scan_batch, acm_select, acm_tally and acm_scan_from on a byte
    machine: the route is the GPU's"""
    m, plan, rec, batch, sel = case
    L, h = m.L, m.handle
    off = np.array(CUTS, np.uint64)

    out, n = _room(2)
    assert L.acm_scan(h, TEXT.ctypes.data, TEXT.size, out.ctypes.data, 2, C.byref(n)) == OVERFLOW and n.value == rec.size
    _same(m.scan_host(TEXT, capacity=rec.size), rec)
    assert m.scan_path == 1

    out, n = _room(2)
    assert L.acm_scan_batch(h, TEXT.ctypes.data, off.ctypes.data, 3, out.ctypes.data, None, None, 2, C.byref(n)) == OVERFLOW and n.value == rec.size
    per_text = m.scan_batch([TEXT[CUTS[t]:CUTS[t + 1]] for t in range(3)], capacity=rec.size)
    assert m.scan_path == 1 and len(per_text) == 3
    for t in range(3):
        want = batch[0][int(batch[2][t]):int(batch[2][t + 1])].copy()
        want["end_pos"] -= CUTS[t]
        _same(per_text[t], want)

    out, n = _room(1)
    assert L.acm_select(h, TEXT.ctypes.data, TEXT.size, out.ctypes.data, 1, C.byref(n)) == OVERFLOW and n.value == rec.size
    _same(m.select(TEXT, capacity=rec.size), sel)
    assert m.scan_path == 1

    want = np.bincount(rec["keyword_id"].astype(np.int64), minlength=len(KEYWORDS)).astype(np.uint64)
    monkeypatch.setenv("ACM_GPU_TALLY_CAPACITY", "2")
    tally, total = m.tally(TEXT)
    assert total == rec.size and np.array_equal(tally, want) and m.scan_path == 1
    monkeypatch.delenv("ACM_GPU_TALLY_CAPACITY")
    tally, total = m.tally(TEXT)
    assert total == rec.size and np.array_equal(tally, want) and m.scan_path == 1

    # acm_scan_from behind a prefix of 5 symbols ("usher"): the cursor is not the root, "hers" lies across
    head, cursor = m.scan_from(m.root(), TEXT[:5])
    _same(head, rec[rec["end_pos"] < 5])
    assert m.scan_path == 1 and cursor.value != m.root().value
    tail = rec[rec["end_pos"] >= 5].copy()
    tail["end_pos"] -= 5
    rest = TEXT[5:]
    out, n = _room(2)
    cur = C.c_void_p(cursor.value)                            # (a copy: the call that follows starts from `cursor` again)
    assert L.acm_scan_from(h, C.byref(cur), rest.ctypes.data, rest.size, out.ctypes.data, 2, C.byref(n)) == OVERFLOW and n.value == tail.size
    got, after = m.scan_from(cursor, rest, capacity=tail.size)
    _same(got, tail)
    assert m.scan_path == 1


def test_stream_finish(case):
    m, plan, rec, batch, sel = case
    s = plan.stream(100, rec.size)
    for at in range(0, TEXT.size, 100):
        s.feed(TEXT[at:at + 100])
    out, n = _room(2)
    rc = acm.lib().acm_gpu_stream_finish(s.h, out.ctypes.data, 2, C.byref(n))
    assert rc == OVERFLOW and n.value == rec.size
    _same(s.finish(), rec)
    s.close()
    plan.status()
