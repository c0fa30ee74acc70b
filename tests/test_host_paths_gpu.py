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
from tests import grep_cases, tally_batch_cases
from tests.batch_cases import oracle_batch
from tests.cases import build_pair
from tests.replace_cases import replace_by_definition
from tests.select_cases import assert_tiling, greedy
from tests.split_cases import expected_offsets
from tests.token_cases import RUN, tokens_by_definition
from tests.words_cases import ASCII_WORD, RIGHT, words

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


def test_plan_tally_batch_host_second_attempt_records(case, monkeypatch):
    """a record room of 2: the first attempt's window overflows, the second attempt's cannot"""
    m, plan, rec, batch, sel = case
    o = build_pair(KEYWORDS, 1)[1]
    off = np.array(CUTS, np.uint64)
    want = tally_batch_cases.expected(o, TEXT, off)
    assert int(want[2].sum()) > 2
    monkeypatch.setenv("ACM_GPU_TALLY_CAPACITY", "2")
    tally_batch_cases.check(plan.tally_batch_host(TEXT, off), want, "capacity 2")
    monkeypatch.delenv("ACM_GPU_TALLY_CAPACITY")
    tally_batch_cases.check(plan.tally_batch_host(TEXT, off), want, "default")
    plan.status()


def test_plan_tally_batch_host_second_attempt_pairs(case, monkeypatch):
    """66,000 texts "he", one (text, keyword) pair each: more pairs than 2^16, fewer records than the
    record room.  With the default record room of 2 Mi the pair room starts at min (2 Mi, n x M) and
    holds them all; the second step makes the record room small, and then both rooms are tried twice."""
    m, plan, rec, batch, sel = case
    monkeypatch.delenv("ACM_GPU_TALLY_CAPACITY", raising=False)
    o = build_pair(KEYWORDS, 1)[1]
    one = o.scan(np.frombuffer(b"he", np.uint8))
    he = KEYWORDS.index(b"he")
    assert one.size == 1 and int(one["keyword_id"][0]) == he                 # one record per text
    n = 66000
    text = np.frombuffer(b"he" * n, np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(2)
    assert n > 65536 and text.size * 1 > 65536 and n < 1 << 21               # more pairs than 2^16, fewer records than 2 Mi

    def check(got):
        assert got.nnz == n and got.total == n
        assert np.array_equal(np.asarray(got.row_ptr).astype(np.uint64), np.arange(n + 1, dtype=np.uint64))
        assert np.all(np.asarray(got.col) == he) and np.all(np.asarray(got.val) == 1)
    check(plan.tally_batch_host(text, off))
    # a record room of 4,096 < 66,000 records: the pair room starts at max (4096, 2^16) = 65,536 < 66,000 pairs, so
    # the record room's second attempt is followed by the pair room's
    monkeypatch.setenv("ACM_GPU_TALLY_CAPACITY", "4096")
    check(plan.tally_batch_host(text, off))
    monkeypatch.delenv("ACM_GPU_TALLY_CAPACITY")
    plan.status()


def test_machine_level_calls_newer(case):
    """acm_replace, acm_tokenize, acm_scan_words, acm_grep, acm_grep_lines and acm_tally_batch on the byte
    machine: with the output room one short ACM_GPU_E_OVERFLOW, the need, and the route is recorded all the
    same; with room exactly the oracle's answer"""
    m, plan, rec, batch, sel = case
    L, h = m.L, m.handle
    o = build_pair(KEYWORDS, 1)[1]
    off = np.array(CUTS, np.uint64)
    texts = [TEXT[CUTS[t]:CUTS[t + 1]] for t in range(3)]
    need, cnt, aux = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def fresh():
        need.value = cnt.value = aux.value = 0

    # acm_replace
    table = [b"<1>", b"", b"two", b"HERS"]
    want = replace_by_definition(TEXT, sel, table)[0]
    data, toff, nk = binding.replacement_table(table, 1)
    out = np.zeros(want.size, np.uint8)
    fresh()
    rc = L.acm_replace(h, TEXT.ctypes.data, TEXT.size, data.ctypes.data, toff.ctypes.data, nk, out.ctypes.data, want.size - 1, C.byref(need), C.byref(cnt))
    assert rc == OVERFLOW and need.value == want.size and cnt.value == sel.size and m.scan_path == 1
    got, k = m.replace(TEXT, table, out_capacity=want.size)
    assert k == sel.size and np.array_equal(got, want) and m.scan_path == 1

    # acm_tokenize
    ids, starts, lens, _ = tokens_by_definition(TEXT, sel, RUN, 1000)
    assert ids.size > sel.size                                               # gap tokens exist
    tid = np.zeros(ids.size, np.uint32)
    fresh()
    rc = L.acm_tokenize(h, TEXT.ctypes.data, TEXT.size, None, 0, None, 0, 1000, RUN, tid.ctypes.data, None, None, ids.size - 1, C.byref(need), None,
                        C.byref(cnt))
    assert rc == OVERFLOW and need.value == ids.size and cnt.value == sel.size and m.scan_path == 1
    tok = m.tokenize(TEXT, mode="run", gap_base=1000, token_capacity=ids.size)
    assert tok.n_tokens == ids.size and tok.count == sel.size and m.scan_path == 1
    assert np.array_equal(tok.ids, ids) and np.array_equal(tok.start, starts) and np.array_equal(tok.length, lens)

    # acm_scan_words: the room must hold all matches
    ww = words(rec, TEXT, flags=RIGHT)
    assert 0 < ww.size < rec.size
    rr, nr = np.asarray(ASCII_WORD, np.uint8).reshape(-1), len(ASCII_WORD)
    out, n = _room(rec.size - 1)
    rc = L.acm_scan_words(h, TEXT.ctypes.data, TEXT.size, rr.ctypes.data, nr, RIGHT, out.ctypes.data, rec.size - 1, C.byref(n))
    assert rc == OVERFLOW and n.value == rec.size and m.scan_path == 1
    _same(m.scan_words(TEXT, flags="right", capacity=rec.size), ww)
    assert m.scan_path == 1

    # acm_grep
    hits = grep_cases.oracle_hits(o, TEXT, off)
    gwant = grep_cases.expected(TEXT, off, hits, False)
    assert 0 < gwant[0].size < 3 and gwant[2].size > 0
    out = np.zeros(gwant[2].size, np.uint8)
    fresh()
    rc = L.acm_grep(h, TEXT.ctypes.data, off.ctypes.data, 3, 0, None, None, C.byref(cnt), C.byref(aux), out.ctypes.data, gwant[2].size - 1, None,
                    C.byref(need))
    assert rc == OVERFLOW and need.value == gwant[2].size and cnt.value == gwant[0].size and aux.value == int(hits.sum()) and m.scan_path == 1
    grep_cases.check(m.grep(texts), hits, gwant, 1, "acm_grep")
    assert m.scan_path == 1

    # acm_grep_lines: cut behind every "r" -- "ushe|r", "sushe|r", ..., "s"
    loff = expected_offsets(TEXT, np.frombuffer(b"r", np.uint8), False)
    lhits = grep_cases.oracle_hits(o, TEXT, loff)
    lwant = grep_cases.expected(TEXT, loff, lhits, False)
    assert loff.size - 1 == 65 and 0 < lwant[0].size < 65
    out = np.zeros(lwant[2].size, np.uint8)
    nt = C.c_uint64(0)
    fresh()
    rc = L.acm_grep_lines(h, TEXT.ctypes.data, TEXT.size, b"r", 1, 0, 0, C.byref(nt), C.byref(cnt), C.byref(aux), out.ctypes.data, lwant[2].size - 1,
                          C.byref(need), 0, None, None, None, None)
    assert rc == OVERFLOW and need.value == lwant[2].size and nt.value == 65 and cnt.value == lwant[0].size and m.scan_path == 1
    got = m.grep_lines(TEXT, delims=b"r")
    assert got.n_texts == 65 and np.array_equal(got.offsets, loff) and m.scan_path == 1
    grep_cases.check(got, lhits, lwant, 1, "acm_grep_lines")

    # acm_tally_batch
    twant = tally_batch_cases.expected(o, TEXT, off)
    k = twant[1].size
    assert k > 1
    row_ptr, col, val = np.zeros(4, np.uint64), np.zeros(k, np.uint32), np.zeros(k, np.uint64)
    fresh()
    rc = L.acm_tally_batch(h, TEXT.ctypes.data, off.ctypes.data, 3, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, k - 1, C.byref(need),
                           C.byref(aux))
    assert rc == OVERFLOW and need.value == k and aux.value == int(twant[2].sum()) and np.array_equal(row_ptr, twant[0]) and m.scan_path == 1
    tally_batch_cases.check(m.tally_batch(texts), twant, "acm_tally_batch")
    assert m.scan_path == 1


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
