"""Flow scans on the GPU (acm_gpu_flows_*, acm_gpu_scan_flows_*, csrc/dev_flows.h) and acm_scan_from on
the GPU paths.  Every test is bit-exact on records, text_id and first, through the device entry and
through the host entry (a Flows object each, fed the same calls), against the ORACLE alone: every
flow's whole history scanned once, its records sliced by piece and rebased (tests/flow_cases.py) --
never the library's own plain or batch scan.  Every workload case first shows from the oracle alone
that it cannot pass trivially: the flow answer has strictly more records than the batch answer of the
same texts, and it is not the scan of a call's buffer as one text.

The workload case of the plan kinds: a text of 2^20 symbols cut at mean 16 has 65,000 pieces, so
"three calls", "257 flows" and "no flow twice in a call" cannot all hold at once.  The case keeps the
text, the cuts, the three calls and the random deal without repeats (three consecutive pieces are one
flow's stream, call c holds piece c of every stream in random order, the streams get random flow
ids) and takes 257 * k flows, k the smallest that gives every stream a flow of its own; the first
3 * 257 pieces are fed once more, in three calls, to exactly 257 flows."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import oracle_batch, random_cuts
from tests.cases import build_pair, build_pair_packed
from tests.flow_cases import (A, B, Cc, D, E, KEYWORDS, N_FLOWS, Call, Reset, boundary_steps, deal, expected, identity_steps, nontrivial,
                              split_scan)
from tests.test_batch_gpu import _check_all, _dev, _kind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _ids(torch, flows):
    return torch.tensor(flows, dtype=torch.int32, device="cuda")


def _feed(torch, plan, n_flows, steps, want, dtype=np.uint8, identity=False, csr=False, what=""):
    """the steps through the device entry and through the host entry, a Flows object each"""
    dev_flows, host_flows = plan.flows(n_flows), plan.flows(n_flows)
    w = iter(want)
    for i, step in enumerate(steps):
        if isinstance(step, Reset):
            dev_flows.reset(None if step.flows is None else _ids(torch, step.flows))
            host_flows.reset(None if step.flows is None else _ids(torch, step.flows))
            continue
        expect = next(w)
        buf = step.buffer(dtype)
        if csr:                                                       # 1 byte past a 16-byte boundary: the CSR walk of a dense plan
            dev = _dev(torch, np.concatenate([np.zeros(1, dtype), buf]))[1:]
            assert dev.data_ptr() % 16 == 1
        else:
            dev = _dev(torch, np.concatenate([buf, np.zeros(16, dtype)]))[:buf.size]
        got = dev_flows.scan(dev, _dev(torch, step.offsets), None if identity else _ids(torch, step.flows))
        _check_all(got, expect, "%s call %d device" % (what, i))
        got = host_flows.scan_host(buf, step.offsets, None if identity else np.array(step.flows, np.uint32))
        _check_all(got, expect, "%s call %d host" % (what, i))
    dev_flows.close()
    host_flows.close()


def test_boundary_set_sparse_ids_short_empty_and_absent_pieces(torch_cuda):
    """1. keywords he, she, hers, s: the carry is 3 symbols.  Five flows over four calls: cuts inside a
    keyword, pieces of one symbol (one carry is assembled from three earlier pieces), empty pieces,
    flows absent from a call; sparse, permuted ids among 300 flows; one scenario with d_flow = NULL"""
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    steps = boundary_steps()
    want = expected(o, steps)
    nontrivial(o, steps, want)
    # what the scenario is there for, from the oracle alone: "hers" ends in the one-symbol piece "s..." of flow C with its full length
    call3 = want[3]
    assert call3[0][0]["end_pos"] == 0 and call3[0][0]["length"] == 4 and call3[1][0] == 0
    _feed(torch_cuda, plan, N_FLOWS, steps, want, what="boundary")
    steps = identity_steps()
    want = expected(o, steps)
    nontrivial(o, steps, want)
    _feed(torch_cuda, plan, 4, steps, want, identity=True, what="identity")
    # no text at all
    f = plan.flows(3)
    _check_all(f.scan_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32)), oracle_batch(o, []))
    _check_all(f.scan(_dev(torch_cuda, np.zeros(16, np.uint8))[:0], _dev(torch_cuda, np.zeros(1, np.uint64)), _ids(torch_cuda, [])),
               oracle_batch(o, []))


KINDS = ("dense", "gram", "csr", "starts", "walk", "u64", "classes", "delta")


@pytest.mark.parametrize("kind,mean", [(k, mean) for k in KINDS for mean in (16, 64)])
def test_every_plan_kind_three_calls_random_deal(torch_cuda, monkeypatch, kat, novel_bytes, kind, mean):
    """2. every plan kind of test_batch_gpu._kind (see the module docstring for the number of flows)"""
    m, o, text, make_plan, plan_ok = _kind(kind, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    if kind == "delta":
        # one keyword longer than every earlier one, in the delta: the carry must follow the delta's lmax
        longest = m.lmax
        at = text.size // 3
        word = text[at:at + 2 * longest + 9].copy()
        m.add_keyword(word)
        o.add_keyword(word)
        plan.update(m)
        assert plan.info.delta_keywords == 151 and plan.info.merges == 0 and word.size > longest
    off = random_cuts(text.size, mean)
    k = (-(-(off.size - 1) // 3) + 256) // 257                       # streams of three pieces, 257 flows at a time
    calls = deal(text, off, 257 * k, 3)
    want = expected(o, calls, text.dtype)
    nontrivial(o, calls, want, text.dtype, every_call=True)
    _feed(torch_cuda, plan, 257 * k, calls, want, text.dtype, csr=kind == "csr", what=kind)
    # exactly 257 flows, three calls, no flow twice in a call
    few = deal(text, off[:3 * 257 + 1], 257, 3, seed=5)
    want = expected(o, few, text.dtype)
    nontrivial(o, few, want, text.dtype)
    _feed(torch_cuda, plan, 257, few, want, text.dtype, csr=kind == "csr", what=kind + " 257")


def test_long_keyword_carried_over_many_pieces(torch_cuda):
    """3. one keyword of 300 symbols, pieces of 1 to 5 symbols: one flow per call in a row of calls, and
    64 flows interleaved"""
    rng = np.random.default_rng(21)
    long_kw = rng.integers(97, 101, size=300).astype(np.uint8)
    kws = [long_kw, long_kw[5:9].copy(), long_kw[100:131].copy(), b"ab", b"c"]
    m, o = build_pair(kws, 1)
    plan = m.plan(0)

    def stream(seed):
        r = np.random.default_rng(seed)
        return np.concatenate([r.integers(97, 101, size=int(r.integers(0, 40))).astype(np.uint8), long_kw,
                               r.integers(97, 101, size=int(r.integers(0, 40))).astype(np.uint8), long_kw[:250], long_kw])

    def pieces(s, seed):
        r = np.random.default_rng(seed)
        cuts, at = [0], 0
        while at < s.size:
            at = min(at + int(r.integers(1, 6)), s.size)
            cuts.append(at)
        return [s[a:b] for a, b in zip(cuts[:-1], cuts[1:])]

    # one flow, one piece per call
    one = [Call([p], [7]) for p in pieces(stream(1), 2)]
    want = expected(o, one)
    nontrivial(o, one, want)
    assert sum(int(np.any(w[0]["length"] == 300)) for w in want) == 2
    _feed(torch_cuda, plan, 9, one[:150], want[:150], what="one flow")            # (the first 150 calls: past the first long match)
    assert any(np.any(w[0]["length"] == 300) for w in want[:150])
    # 64 flows interleaved: call c holds piece c of every flow that still has one
    per_flow = [pieces(stream(100 + f), 200 + f) for f in range(64)]
    many = []
    for c in range(max(len(p) for p in per_flow)):
        fl = [f for f in range(64) if c < len(per_flow[f])]
        many.append(Call([per_flow[f][c] for f in fl], [(f * 37) % 64 for f in fl]))
    want = expected(o, many)
    nontrivial(o, many, want)
    assert sum(int(np.sum(w[0]["length"] == 300)) for w in want) == 128
    _feed(torch_cuda, plan, 64, many, want, what="64 flows")


def test_dictionary_of_single_symbols_has_an_empty_carry(torch_cuda):
    """4. lmax = 1: nothing is carried, the answer is the batch's"""
    m, o = build_pair([b"a", b"s", b"e"], 1)
    plan = m.plan(0)
    text = np.frombuffer(b"she sells sea shells" * 40, np.uint8)
    off = random_cuts(text.size, 8)
    calls = deal(text, off, 257, 2)
    want = expected(o, calls)
    for c, w in zip(calls, want):
        _check_all(w, oracle_batch(o, c.texts), "oracle")
    assert sum(w[0].size for w in want) > 100
    _feed(torch_cuda, plan, 257, calls, want, what="lmax 1")


def _device_call(torch, plan, flows, dev, off_dev, flow_dev, cap):
    L = acm.lib()
    n_sym, n_texts = dev.numel() * dev.element_size() // plan.sym_size, off_dev.numel() - 1
    rec = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device="cuda")
    tid = torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda")
    first = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_scan_flows_tmp_bytes(plan.h, flows.h, cap, n_sym, n_texts)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_scan_flows_device(plan.h, flows.h, dev.data_ptr(), n_sym, off_dev.data_ptr(), flow_dev.data_ptr() if flow_dev is not None else None,
                                     n_texts, rec.data_ptr(), tid.data_ptr(), first.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), tb, None)
    torch.cuda.synchronize()
    n = int(cnt.item())
    got = None
    if rc == 0 and n <= cap:
        got = (np.frombuffer(rec[:n].cpu().numpy().tobytes(), dtype=binding.RECORD_DTYPE), tid[:n].cpu().numpy().view(np.uint32),
               first.cpu().numpy().view(np.uint64))
    return rc, n, got


def _synthetic_calls(n, mean, n_calls, n_flows):
    kd, ko = acm.synth.keywords(1000)
    m, o = build_pair_packed(kd, ko)
    text = acm.synth.text(n, kd, ko)
    calls = deal(text, random_cuts(n, mean), n_flows, n_calls)
    return m, o, calls


def test_overflow_leaves_the_carries_and_a_capacity_that_suffices(torch_cuda):
    """5. a call with too little room leaves *d_count > capacity; the same call with that count as the
    capacity gives the oracle's answer: the carries were not advanced"""
    m, o, calls = _synthetic_calls(1 << 16, 64, 2, 600)
    want = expected(o, calls)
    nontrivial(o, calls, want)
    plan = m.plan(0)
    flows = plan.flows(600)
    args = [(_dev(torch_cuda, c.buffer(np.uint8)), _dev(torch_cuda, c.offsets), _ids(torch_cuda, c.flows)) for c in calls]
    rc, n, got = _device_call(torch_cuda, plan, flows, *args[0], cap=want[0][0].size + 4096)
    assert rc == 0
    _check_all(got, want[0], "first call")
    need = None
    for cap in (0, 1, want[1][0].size - 1):
        rc, n, got = _device_call(torch_cuda, plan, flows, *args[1], cap=cap)
        assert rc == 0 and n > cap and got is None, (cap, rc, n)
        need = n
    rc, n, got = _device_call(torch_cuda, plan, flows, *args[1], cap=need)
    assert rc == 0 and n == want[1][0].size
    _check_all(got, want[1], "after overflow")
    plan.status()
    # the host entry says so with its return value and leaves the carries as well
    hflows = plan.flows(600)
    _check_all(hflows.scan_host(calls[0].buffer(np.uint8), calls[0].offsets, np.array(calls[0].flows, np.uint32)), want[0], "host first")
    rec = np.zeros(4, binding.RECORD_DTYPE)
    nf = C.c_uint64(0)
    buf, fl = calls[1].buffer(np.uint8), np.array(calls[1].flows, np.uint32)
    rc = acm.lib().acm_gpu_scan_flows_host(plan.h, hflows.h, buf.ctypes.data, buf.size, calls[1].offsets.ctypes.data, fl.ctypes.data, fl.size,
                                           rec.ctypes.data, None, None, 4, C.byref(nf))
    assert rc == binding.ACM_GPU_E_OVERFLOW and nf.value > 4
    _check_all(hflows.scan_host(buf, calls[1].offsets, fl, capacity=7), want[1], "host retry")


def test_bad_flow_ids_are_flagged_report_nothing_and_leave_the_carries(torch_cuda):
    """6. a duplicate flow id and an id >= n_flows through the device entry: *d_count == 0, the plan's
    status raises, and a following valid call still gives the oracle's answer; the same inputs through
    the host entry are ACM_GPU_E_ARG"""
    m, o, calls = _synthetic_calls(1 << 16, 64, 2, 600)
    want = expected(o, calls)
    nontrivial(o, calls, want)
    good = np.array(calls[1].flows, np.uint32)
    for what in ("duplicate", "range"):
        plan = m.plan(0)
        flows = plan.flows(600)
        c0 = calls[0]
        rc, n, got = _device_call(torch_cuda, plan, flows, _dev(torch_cuda, c0.buffer(np.uint8)), _dev(torch_cuda, c0.offsets),
                                  _ids(torch_cuda, c0.flows), cap=want[0][0].size + 4096)
        assert rc == 0
        _check_all(got, want[0], what + " first call")
        plan.status()
        bad = good.copy()
        if what == "duplicate":
            bad[good.size // 2] = bad[5]
        else:
            bad[good.size // 2] = 600
        c1 = calls[1]
        dev, off_dev = _dev(torch_cuda, c1.buffer(np.uint8)), _dev(torch_cuda, c1.offsets)
        rc, n, got = _device_call(torch_cuda, plan, flows, dev, off_dev, _ids(torch_cuda, bad.astype(np.int64).tolist()), cap=1 << 16)
        assert rc == 0 and n == 0, (what, rc, n)
        with pytest.raises(binding.ACMError) as e:
            plan.status()
        assert e.value.code == -7, what
        # the carries are untouched: the valid call gives the oracle's answer (the flag of the plan stays up until the plan goes)
        rc, n, got = _device_call(torch_cuda, plan, flows, dev, off_dev, _ids(torch_cuda, good.astype(np.int64).tolist()), cap=1 << 16)
        assert rc == 0
        _check_all(got, want[1], what + " valid call after the bad one")
        nf = C.c_uint64(0)
        rec = np.zeros(1 << 16, binding.RECORD_DTYPE)
        buf = c1.buffer(np.uint8)
        assert acm.lib().acm_gpu_scan_flows_host(plan.h, flows.h, buf.ctypes.data, buf.size, c1.offsets.ctypes.data, bad.ctypes.data, bad.size,
                                                 rec.ctypes.data, None, None, 1 << 16, C.byref(nf)) == binding.ACM_GPU_E_ARG
    # flows of another plan, too little scratch, more texts than flows without ids
    plan, other = m.plan(0), m.plan(0)
    flows = plan.flows(8)
    L = acm.lib()
    cnt = torch_cuda.zeros(1, dtype=torch_cuda.int64, device="cuda")
    c1 = calls[1]
    dev, off_dev = _dev(torch_cuda, c1.buffer(np.uint8)), _dev(torch_cuda, c1.offsets)
    assert L.acm_gpu_scan_flows_device(other.h, flows.h, dev.data_ptr(), dev.numel(), off_dev.data_ptr(), None, 4, None, None, None, 0,
                                       cnt.data_ptr(), dev.data_ptr(), dev.numel(), None) == binding.ACM_GPU_E_ARG
    assert L.acm_gpu_scan_flows_device(plan.h, flows.h, dev.data_ptr(), dev.numel(), off_dev.data_ptr(), None, off_dev.numel() - 1, None, None,
                                       None, 0, cnt.data_ptr(), dev.data_ptr(), dev.numel(), None) == binding.ACM_GPU_E_ARG
    assert L.acm_gpu_scan_flows_device(plan.h, flows.h, dev.data_ptr(), dev.numel(), off_dev.data_ptr(), _ids(torch_cuda, c1.flows).data_ptr(),
                                       off_dev.numel() - 1, None, None, None, 0, cnt.data_ptr(), dev.data_ptr(), 16, None) == binding.ACM_GPU_E_ARG
    plan.status()


def test_a_longer_keyword_than_the_slots_hold_is_refused(torch_cuda):
    """the slot width is fixed when the flows are made: an update that brings a longer keyword makes
    the next flow scan ACM_GPU_E_ARG, never a scan with a short carry"""
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    flows = plan.flows(4)
    m.add_keyword(b"a keyword far longer than sixteen bytes of slot")
    plan.update(m)
    with pytest.raises(binding.ACMError) as e:
        flows.scan_host(np.frombuffer(b"ushers", np.uint8), np.array([0, 6], np.uint64), np.array([1], np.uint32))
    assert e.value.code == binding.ACM_GPU_E_ARG
    fresh = plan.flows(4)
    got = fresh.scan_host(np.frombuffer(b"ushers", np.uint8), np.array([0, 6], np.uint64), np.array([1], np.uint32))
    assert np.array_equal(got[0], o.scan(b"ushers"))


def test_reset_of_some_flows_between_calls(torch_cuda):
    """7. the flows that were reset restart from the root, the others continue"""
    m, o = build_pair(KEYWORDS, 1)
    plan = m.plan(0)
    steps = [Call([b"us", b"ush", b"sh", b"he"], [A, B, Cc, D]), Reset([B, D]), Call([b"hers", b"ers", b"e", b"rs"], [A, B, Cc, D]),
             Reset(), Call([b"ers", b"e"], [A, Cc])]
    want = expected(o, steps)
    nontrivial(o, steps, want)
    # from the oracle alone: A and C continue ("she" ends in A's "hers", in C's "e"), B and D restart ("ers", "rs": an "s" each)
    rec, tid, first = want[1]
    assert np.array_equal(rec[tid == 0]["length"], [3, 2, 4, 1]) and np.array_equal(rec[tid == 2]["length"], [3, 2])
    assert np.array_equal(rec[tid == 1]["length"], [1]) and np.array_equal(rec[tid == 3]["length"], [1])
    assert np.array_equal(want[2][0]["length"], [1])                 # after the reset of all: "ers" alone, "e" alone
    _feed(torch_cuda, plan, N_FLOWS, steps, want, what="reset")


def test_scan_from_on_the_gpu_paths(torch_cuda, kat, novel_bytes):
    """8. acm_scan_from on ACM_SCAN_PATH_GPU and ACM_SCAN_PATH_GPU_CLASSES (wchar_t + alphacmp): a prefix
    fed symbol by symbol, a bulk middle, a tail fed symbol by symbol, on the novel with the reference's
    word list, against the oracle's single loop"""
    words = (b"He", b"SHE", b"his", b"hErs", b"Mrs", b"dalloway")
    L = acm.lib()
    for sym, cmp_name, dt, path in ((1, None, np.uint8, 1), (4, "kat_casecmp32", np.uint32, 2), (1, "kat_casecmp8", np.uint8, 2)):
        cmp = C.cast(getattr(kat, cmp_name), C.c_void_p) if cmp_name else None
        m = acm.Machine(sym, cmp=cmp)
        o = po.Oracle(sym, po.MEYER85, cmp=cmp) if cmp_name else po.Oracle(sym, po.MEYER85)
        for kw in words:
            w = np.frombuffer(kw if cmp_name else kw.lower(), np.uint8).astype(dt)
            m.add_keyword(w)
            o.add_keyword(w)
        if cmp_name:
            m.set_symbol_bytes(sym)
        text = np.frombuffer(novel_bytes[:60000], np.uint8).astype(dt)
        want = o.scan(text)
        assert want.size > 1500
        # cuts inside a match: right behind the first symbol of a record of length >= 3, and before its last
        r = want[want["length"] >= 3][40]
        a = int(r["end_pos"]) - int(r["length"]) + 2
        r = want[(want["length"] >= 3) & (want["end_pos"] > a + 30000)][0]
        b = int(r["end_pos"])
        for (lo, hi) in ((a, b), (0, b), (a, text.size), (a, a), (a, a + 1)):
            lo_start = max(lo - 200, 0)                               # (the per-symbol parts are slow through ctypes: 200 symbols each)
            part = text[lo_start:min(hi + 200, text.size)].copy()
            w = o.scan(part)                                          # the oracle's single loop over what is fed
            split_scan(L, m.handle, part, sym, lo - lo_start, hi - lo_start, np.bincount(w["end_pos"].astype(np.int64), minlength=part.size), w)
            assert m.scan_path == path
        # the Python wrapper: two halves from the root
        first, cur = m.scan_from(m.root(), text[:a])
        second, cur = m.scan_from(cur, text[a:])
        second = second.copy()
        second["end_pos"] += np.uint64(a)
        assert np.array_equal(np.concatenate([first, second]), want)
