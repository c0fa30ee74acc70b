"""Shared by tests/test_streams_gpu.py: every acm_gpu_* entry point of include/acm_gpu.h that takes a `void *stream`,
as a raw call through binding.lib () with caller-owned buffers, and the machinery that runs such a call behind a gate.

A Case names the inputs that decide the answer (`gated`: name -> (real, decoy), same shape and type), the outputs, the
scratch of exactly *_tmp_bytes and the part of every output that counts (`cut`).  A Run holds them on the device and
runs the call
    plain    on the null stream, synchronised: the expected value, held against Case.want -- the oracle's records and the
             definitions of tests/*_cases.py, output by output (None: an output without a definition);
    early    the buffers hold the decoy, scratch and outputs are zero; on a non-blocking side stream a gate
             (torch.cuda._sleep), the copy of the real inputs and the call, the null stream idle: whatever the call
             launches on stream 0 runs during the gate, on the decoy and on empty scratch;
    late     scratch and outputs as a call on the decoy left them, the gate on the null stream, copy and call on the side
             stream: whatever the call launches on stream 0 sits behind the gate, and the stages behind it read what the
             decoy left;
    control  early, but the call is handed the null stream: it must give the DECOY's answer -- the proof that the gate
             is long enough and the two streams do not wait for each other.
early and late also say whether the call came back while the gate was still running (no host round trip)."""
import ctypes as C
import os
import re
import time

import numpy as np

from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests import approx_cases, chain_cases, context_cases, edit_cases, flow_cases, grep_cases, pattern_cases, replace_cases, rules_cases
from tests import split_cases, template_cases, token_cases, words_cases
from tests.select_cases import greedy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "acm_gpu.h")
OK = binding.ACM_GPU_OK
REC = po.RECORD_DTYPE


def header_stream_functions(path=HEADER):
    """the functions include/acm_gpu.h declares with a `void *stream` parameter, in order"""
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", src) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))]


PLAIN = ["acm_gpu_scan_device", "acm_gpu_count_device", "acm_gpu_scan_ordered_device", "acm_gpu_order_records_device",
         "acm_gpu_sort_records_device", "acm_gpu_pack_records_device", "acm_gpu_unpack_records_device"]
EXCLUDED = {
    "acm_gpu_comm_gather_records": "needs RCCL peers, one rank per device; tests/test_gpu_parity.py runs it with ranks as threads over the loopback transport",
}


# ---------------------------------------------------------------------------------------------- the gate
class Gates:
    """the side stream and torch.cuda._sleep calibrated in cycles per millisecond on this device"""

    def __init__(self, torch):
        self.torch = torch
        self.side = torch.cuda.Stream()                  # (torch creates its streams non-blocking)
        assert self.side.cuda_stream != 0 and torch.cuda.default_stream().cuda_stream == 0
        torch.cuda._sleep(100000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 1000000
        while True:
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0 or cycles >= 10 ** 11:
                break
            cycles *= 8
        self.cycles_per_ms = cycles / ms
        self.longest_plain_ms = 0.0
        self.longest_gate_ms = 0.0
        print("gate: %d cycles took %.3f ms: %.0f cycles per ms" % (cycles, ms, self.cycles_per_ms))

    def length_ms(self, plain_ms):
        """100 ms, or 50 times the wall time of the plain call with its synchronise; more than 1 s is refused"""
        self.longest_plain_ms = max(self.longest_plain_ms, plain_ms)
        ms = max(100.0, 50.0 * plain_ms)
        assert ms <= 1000.0, "too slow for its shape: the plain call took %.2f ms" % plain_ms
        self.longest_gate_ms = max(self.longest_gate_ms, ms)
        return ms

    def sleep(self, ms):
        self.torch.cuda._sleep(int(self.cycles_per_ms * ms))


# ---------------------------------------------------------------------------------------------- a case and its runs
class Case:
    def __init__(self, name, plan, call, gated, outs, tmp_bytes=0, cut=None, prepare=None, post=None, accumulate=(), misalign=(), want=None,
                 keep=()):
        self.name, self.plan, self.call, self.gated, self.outs, self.tmp_bytes = name, plan, call, gated, outs, int(tmp_bytes)
        self.cut = cut if cut is not None else (lambda h: [h[k] for k in outs])
        self.prepare, self.post, self.accumulate, self.misalign, self.want, self.keep = prepare, post, tuple(accumulate), tuple(misalign), want, keep


def flat(a):
    """a numpy array as the flat array of signed integers torch takes (records become pairs of int64)"""
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.int64)
    return a.reshape(-1).view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def dev(torch, a):
    a = flat(a)
    return torch.from_numpy(a.copy() if a.size else np.zeros(1, a.dtype)).cuda()


def same(got, want):
    return len(got) == len(want) and all(np.asarray(g).shape == np.asarray(w).shape and np.array_equal(g, w) for g, w in zip(got, want))


def show(arrays):
    return [(np.asarray(a).shape, np.asarray(a).reshape(-1)[:6].tolist()) for a in arrays]


class Run:
    def __init__(self, torch, gates, case):
        self.torch, self.gates, self.case = torch, gates, case
        self.b, self.src = {}, {"real": {}, "decoy": {}}
        for name, (real, decoy) in case.gated.items():
            r, d = flat(real), flat(decoy)
            assert r.shape == d.shape and r.dtype == d.dtype and r.size > 0, name
            assert not np.array_equal(r, d) or len(case.gated) > 1, name
            self.src["real"][name], self.src["decoy"][name] = dev(torch, r), dev(torch, d)
            if name in case.misalign:                    # one byte behind a 16-byte boundary
                assert r.dtype == np.uint8
                self.b[name] = torch.zeros(r.size + 16, dtype=torch.uint8, device="cuda")[1:1 + r.size]
                assert self.b[name].data_ptr() % 16 == 1
            else:
                self.b[name] = torch.zeros_like(self.src["real"][name])
        for name, (count, dtype) in case.outs.items():
            self.b[name] = torch.zeros(max(int(count), 1), dtype=dtype, device="cuda")
        self.tmp = torch.zeros(max(case.tmp_bytes, 16), dtype=torch.uint8, device="cuda")
        self.p = {k: v.data_ptr() for k, v in self.b.items()}
        self.p["tmp"] = self.tmp.data_ptr()
        torch.cuda.synchronize()

    # -- pieces
    def _load(self, which):
        for name in self.case.gated:
            self.b[name].copy_(self.src[which][name])

    def _zero(self, everything):
        for name in (self.case.outs if everything else self.case.accumulate):
            self.b[name].zero_()
        if everything:
            self.tmp.zero_()

    def _host(self, bufs):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    def _begin(self, scratch_zero):
        torch, c = self.torch, self.case
        torch.cuda.synchronize()
        if c.prepare:
            c.prepare(self.p)
        self._load("decoy")
        self._zero(scratch_zero)
        torch.cuda.synchronize()

    def _end(self, rc):
        torch, c = self.torch, self.case
        if c.post:
            c.post(self.p, None)
        torch.cuda.synchronize()
        assert rc == OK, (c.name, rc)
        c.plan.status()                                  # (waits for the device; raises when a kernel flagged an error)
        return c.cut(self._host(self.b))

    # -- the arrangements
    def plain(self, which):
        """the call on the null stream, synchronised: (what counts of its outputs, wall milliseconds)"""
        torch, c = self.torch, self.case
        torch.cuda.synchronize()
        if c.prepare:
            c.prepare(self.p)
        self._load(which)
        self._zero(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = c.call(self.p, None)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return self._end(rc), ms

    def early(self, gate_ms):
        """(outputs, the call returned while the gate was still running and left its stream busy)"""
        torch, side = self.torch, self.gates.side
        self._begin(True)
        gate_done = torch.cuda.Event()
        with torch.cuda.stream(side):
            self.gates.sleep(gate_ms)
            gate_done.record()
            self._load("real")
            rc = self.case.call(self.p, side.cuda_stream)
            asynchronous = (not gate_done.query()) and (not side.query())
        side.synchronize()
        return self._end(rc), asynchronous

    def late(self, gate_ms):
        """(outputs, the side stream drained while the null stream was still behind its gate); call plain ("decoy") first"""
        torch, side = self.torch, self.gates.side
        self._begin(False)
        self.gates.sleep(gate_ms)                        # on the null stream
        with torch.cuda.stream(side):
            self._load("real")
            rc = self.case.call(self.p, side.cuda_stream)
        side.synchronize()
        independent = not torch.cuda.default_stream().query()
        torch.cuda.synchronize()
        return self._end(rc), independent

    def control(self, gate_ms):
        """early with the call on the null stream: what it left there, taken on the null stream right behind it"""
        torch, side, c = self.torch, self.gates.side, self.case
        self._begin(True)
        with torch.cuda.stream(side):
            self.gates.sleep(gate_ms)
            self._load("real")
        rc = c.call(self.p, None)
        if c.post:
            c.post(self.p, None)
        snap = {k: v.clone() for k, v in self.b.items()}
        torch.cuda.synchronize()                         # before anything else touches the plan
        assert rc == OK, (c.name, rc)
        c.plan.status()
        return c.cut({k: v.cpu().numpy() for k, v in snap.items()})


def exercise(torch, gates, case, control=False):
    """the arrangements of one case; returns the failures as strings (none: the case passes)"""
    run = Run(torch, gates, case)
    want, _ = run.plain("real")                          # grows the plan's lazily allocated buffers
    decoy, plain_ms = run.plain("decoy")                 # warm: the wall time the gate goes by
    assert not same(want, decoy), (case.name, "the decoy gives the real answer", show(want))
    assert np.asarray(want[0]).size > 0 and any(np.any(np.asarray(a) != 0) for a in want), (case.name, "an empty answer", show(want))
    if case.want is not None:                            # (None: an output the case has no expected value of its own for)
        for i, w in enumerate(case.want):
            assert w is None or same([want[i]], [w]), (case.name, "plain call against the oracle", i, show([want[i]]), show([w]))
    again, _ = run.plain("real")
    assert same(again, want), (case.name, "two plain calls differ", show(again), show(want))
    gate_ms = gates.length_ms(plain_ms)
    print("%s: plain call %.3f ms, gate %.0f ms" % (case.name, plain_ms, gate_ms))
    bad = []
    got, asynchronous = run.early(gate_ms)
    if not same(got, want):
        bad.append("%s early: wrong answer %s, want %s%s" % (case.name, show(got), show(want), " (the decoy's)" if same(got, decoy) else ""))
    if not asynchronous:
        bad.append("%s early: the call waited for its stream" % case.name)
    run.plain("decoy")
    got, independent = run.late(gate_ms)
    if not same(got, want):
        bad.append("%s late: wrong answer %s, want %s%s" % (case.name, show(got), show(want), " (the decoy's)" if same(got, decoy) else ""))
    if not independent:
        bad.append("%s late: the side stream waited for the null stream" % case.name)
    if control:
        got = run.control(gate_ms)
        if same(got, want):
            raise RuntimeError("%s control: gate too short or streams not independent" % case.name)
        if not same(got, decoy):
            bad.append("%s control: neither answer %s, decoy %s" % (case.name, show(got), show(decoy)))
        else:
            print("%s control: the decoy's answer" % case.name)
    return bad


# ---------------------------------------------------------------------------------------------- helpers of the cases
def rows(h, name, n=None):
    a = h[name].reshape(-1, 2)
    return a if n is None else a[:int(n)]


def sorted_rows(a):
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def rec_rows(rec):
    return flat(rec).reshape(-1, 2)


def padded(rec, room):
    a = np.zeros(room, REC)
    a[:rec.size] = rec
    return a


def terms_of(terms, ptr):
    """a set's flat terms[] as one list of (keyword_id, x, y) per member, by its ptr[] array"""
    return [[tuple(int(x) for x in terms[i]) for i in range(int(ptr[c]), int(ptr[c + 1]))] for c in range(len(ptr) - 1)]


def i32(a):
    """values below 2^32 as the int32 a device buffer of uint32_t comes back as"""
    return np.asarray(a).astype(np.uint32).view(np.int32)


def i64(a):
    return np.asarray(a).astype(np.uint64).view(np.int64)


def batch_records(o, text, off):
    """the oracle's records of every text scanned on its own, end_pos = the index in the buffer"""
    parts = []
    for t in range(off.size - 1):
        lo, hi = int(off[t]), int(off[t + 1])
        if hi > lo:
            r = o.scan(text[lo:hi]).copy()
            r["end_pos"] += lo
            parts.append(r)
    return np.concatenate(parts) if parts else np.zeros(0, REC)


PLAIN_BY_PLAN = {
    "acm_gpu_pack_records_device": "the packed word goes by acm_gpu_wire_bits (plan, ...): no expected value without a plan",
    "acm_gpu_unpack_records_device": "its input is packed by acm_gpu_wire_bits (plan, ...): no expected value without a plan",
}


def plain_expected(o, real, decoy, which="real"):
    """{entry point: expected outputs} of the plain entry points whose answer the oracle alone gives (not PLAIN_BY_PLAN's),
    for the `real` or the `decoy` text: the scans give the oracle's records, the two sorts the first m of them, m = the
    smaller number of records of the two texts"""
    both = {"real": o.scan(real), "decoy": o.scan(decoy)}
    m = min(both["real"].size, both["decoy"].size)
    w = both[which]
    return {"acm_gpu_scan_device": [sorted_rows(rec_rows(w)), np.array([w.size])],
            "acm_gpu_count_device": [np.array([w.size])],
            "acm_gpu_scan_ordered_device": [rec_rows(w), np.array([w.size])],
            "acm_gpu_order_records_device": [rec_rows(w[:m])],
            "acm_gpu_sort_records_device": [rec_rows(w[:m])]}


def plain_cases(torch, plan, o, real, decoy, misalign=False):
    """the seven plain entry points on one plan: `real` and `decoy` are two texts of one length"""
    import torch as T
    L, h, sb = binding.lib(), plan.h, plan.sym_size
    n = real.size
    assert decoy.size == n and real.dtype == decoy.dtype and real.dtype.itemsize == sb
    want, other = o.scan(real), o.scan(decoy)
    cap = max(want.size, other.size) + 64
    m = min(want.size, other.size)
    # on the CPU, by the oracle: non-empty, different, inside the capacity
    assert m >= 64 and not np.array_equal(want[:m], other[:m]) and want.size != other.size, (want.size, other.size)
    by_oracle = plain_expected(o, real, decoy)
    text = {"text": (real.view(np.uint8) if misalign else real, decoy.view(np.uint8) if misalign else decoy)}
    mis = ("text",) if misalign else ()
    cases = []
    cases.append(Case("acm_gpu_scan_device", plan,
                      lambda p, st: L.acm_gpu_scan_device(h, p["text"], n, 0, 0, p["rec"], cap, p["count"], st),
                      text, {"rec": (2 * cap, T.int64), "count": (1, T.int64)}, misalign=mis,
                      cut=lambda x: [sorted_rows(rows(x, "rec", min(x["count"][0], cap))), x["count"]],      # (in no particular order)
                      want=by_oracle["acm_gpu_scan_device"]))
    cases.append(Case("acm_gpu_count_device", plan,
                      lambda p, st: L.acm_gpu_count_device(h, p["text"], n, 0, p["count"], st),
                      text, {"count": (1, T.int64)}, misalign=mis, want=by_oracle["acm_gpu_count_device"]))
    cases.append(Case("acm_gpu_scan_ordered_device", plan,
                      lambda p, st: L.acm_gpu_scan_ordered_device(h, p["text"], n, 0, 0, p["rec"], cap, p["count"], p["tmp"], tb_ordered, st),
                      text, {"rec": (2 * cap, T.int64), "count": (1, T.int64)}, misalign=mis,
                      tmp_bytes=L.acm_gpu_scan_ordered_tmp_bytes(h, cap, n),
                      cut=lambda x: [rows(x, "rec", min(x["count"][0], cap)), x["count"]],
                      want=by_oracle["acm_gpu_scan_ordered_device"]))
    tb_ordered = cases[-1].tmp_bytes
    # the records of both texts cut to one number and shuffled: a prefix of a canonical record set is one
    perm = np.random.default_rng(5).permutation(m)
    shuffled = {"rec": (want[:m][perm], other[:m][perm])}
    tb_order, tb_sort = L.acm_gpu_order_tmp_bytes(h, m, n), L.acm_gpu_sort_tmp_bytes(m)
    cases.append(Case("acm_gpu_order_records_device", plan,
                      lambda p, st: L.acm_gpu_order_records_device(h, p["rec"], m, 0, n, p["tmp"], tb_order, st),
                      shuffled, {}, tmp_bytes=tb_order, cut=lambda x: [rows(x, "rec")], want=by_oracle["acm_gpu_order_records_device"]))
    cases.append(Case("acm_gpu_sort_records_device", plan,
                      lambda p, st: L.acm_gpu_sort_records_device(h, p["rec"], m, p["tmp"], tb_sort, st),
                      shuffled, {}, tmp_bytes=tb_sort, cut=lambda x: [rows(x, "rec")], want=by_oracle["acm_gpu_sort_records_device"]))
    bits = [C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)]
    assert L.acm_gpu_wire_bits(h, n, *[C.byref(x) for x in bits]) == 0
    pb, lb = bits[0].value, bits[1].value

    def pack(r):
        return r["end_pos"] | (r["length"].astype(np.uint64) << np.uint64(pb)) | (r["keyword_id"].astype(np.uint64) << np.uint64(pb + lb))
    cases.append(Case("acm_gpu_pack_records_device", plan,
                      lambda p, st: L.acm_gpu_pack_records_device(p["rec"], m, 0, pb, lb, p["packed"], st),
                      {"rec": (want[:m], other[:m])}, {"packed": (m, T.int64)}, want=[flat(pack(want[:m]))]))
    cases.append(Case("acm_gpu_unpack_records_device", plan,
                      lambda p, st: L.acm_gpu_unpack_records_device(p["packed"], m, 0, pb, lb, p["rec"], st),
                      {"packed": (pack(want[:m]), pack(other[:m]))}, {"rec": (2 * m, T.int64)}, cut=lambda x: [rows(x, "rec")],
                      want=[rec_rows(want[:m])]))
    assert [c.name for c in cases] == PLAIN
    return cases


# ---------------------------------------------------------------------------------------------- the feature entry points
CAP = 2048                                               # records: the room of every record buffer of the feature cases
WINDOW = 1024                                            # symbols per window of the windowed calls: four windows


class Features:
    """One plan, one batch (text and decoy text of N symbols under one offsets[] of T texts), the sets of the
    set families built from the two keywords of two symbols or more that the real text holds most often, a Case per
    entry point and, without a device, what each of them must give: expected (name, "real" or "decoy"), from the oracle's
    records and the families' definitions in plain Python.  torch None: no plan and no device buffers, expected () alone."""

    def __init__(self, torch, m, o, make_plan, real, decoy, off, word_ranges=binding.ASCII_WORD, trailing=None, last_step=None):
        """trailing: a keyword no set refers to, added to machine and oracle behind the sets' pieces.  last_step (features):
        called once self.plan is there, in front of the first case -- a plan maker that has one step of growth left compiles
        the sets on the plan as it is and then grows it (tests/growth_cases.py)."""
        self.torch, self.m, self.o = torch, m, o
        self.real, self.decoy, self.off = np.ascontiguousarray(real), np.ascontiguousarray(decoy), np.ascontiguousarray(off, dtype=np.uint64)
        self.N, self.T = self.real.size, self.off.size - 1
        assert self.decoy.size == self.N and int(self.off[-1]) == self.N and self.real.dtype == np.uint8
        # the two keywords the real batch holds most often (by the oracle), and the sets made of them
        rec = batch_records(o, self.real, self.off)
        ids, counts = np.unique(rec["keyword_id"], return_counts=True)
        order = [int(ids[i]) for i in np.argsort(-counts, kind="stable") if len(m.keyword(int(ids[i]))[0]) >= 2]    # (of two symbols or more)
        a, b = order[0], order[1]
        sa, sb = [int(x) for x in m.keyword(a)[0]], [int(x) for x in m.keyword(b)[0]]
        la, lb = len(sa), len(sb)
        assert la >= 2 and lb >= 2
        self.patternset = binding.PatternSet([[(a, 0, la)], [(b, 0, lb)], [(a, 0, la), (b, la + 2, lb)]])
        self.chainset = binding.ChainSet([[(a, 0, 0), (b, 0, 40)], [(b, 0, 0), (a, 1, 25)]])
        self.ruleset = binding.RuleSet([binding.rule([binding.present(a)]), binding.rule([binding.present(b), binding.absent(a)]),
                                        binding.rule([binding.present(a, 2), binding.present(b, 2)], need=1)])
        before = m.nb_keywords
        self.targets, self.target_k = [bytes(sa + sb), bytes(sb + [sa[0]])], [1, 1]
        self.approxset = binding.ApproxSet.from_targets(m, self.targets, 1)
        cells = list(sa)
        cells[1] = binding.SymbolClass([(sa[1] - 1, sa[1] + 1)])
        self.templates, self.template_k = [cells, sb + [binding.ANY] + sa], [0, 1]
        self.templateset = binding.TemplateSet.from_templates(m, self.templates, k=self.template_k)
        if trailing is not None:
            m.add_keyword(trailing)
        for k in range(before, m.nb_keywords):           # the pieces the two sets added (and the trailing keyword), into the oracle as well
            o.add_keyword(bytes(m.keyword(k)[0]))
        assert o.nb_keywords == m.nb_keywords
        self.K = m.nb_keywords
        self.word_ranges = tuple(word_ranges)
        self.handles = {}
        self.plan = None
        if torch is not None:
            self.plan = make_plan(0)
            if last_step is not None:
                last_step(self)
            assert self.plan.tally_keywords == self.K
        # on the CPU, by the oracle: the records of both batches are there, differ and fit the room
        self.rec, self.rec_decoy = batch_records(o, self.real, self.off), batch_records(o, self.decoy, self.off)
        whole, whole_decoy = o.scan(self.real).size, o.scan(self.decoy).size
        self.n = min(self.rec.size, self.rec_decoy.size)
        assert 64 <= self.n and max(whole, whole_decoy) <= CAP // 2 and not np.array_equal(self.rec[:self.n], self.rec_decoy[:self.n])
        self.sel, self.sel_decoy = binding.select_records(self.rec), binding.select_records(self.rec_decoy)
        self.ns = min(self.sel.size, self.sel_decoy.size)
        assert 32 <= self.ns < self.n and not np.array_equal(self.sel[:self.ns], self.sel_decoy[:self.ns])
        self.whole = {"real": o.scan(self.real), "decoy": o.scan(self.decoy)}
        self.ranges, self.n_ranges = binding._word_ranges(word_ranges, 1)
        self.delim = int(np.bincount(self.real).argmax())
        self.delims, self.n_delims = binding._delims(bytes([self.delim]), 1)
        self.pre_text = np.roll(self.decoy, 977)         # what every flow is fed in front of a flow case's call
        repl = [b"<%d>" % k if k % 2 else b"" for k in range(self.K)]
        data, roff = binding.replacement_table(repl, 1)[:2]
        self.repl = repl
        self.keep = []
        self.wants = {}
        if torch is not None:
            self.d_off, self.d_repl, self.d_repl_off = dev(torch, self.off), dev(torch, data), dev(torch, roff)

    def handle(self, family):
        if family not in self.handles:
            p = self.plan
            self.handles[family] = {"rules": lambda: p.rules_create(self.ruleset), "patterns": lambda: p.patterns_create(self.patternset),
                                    "chains": lambda: p.chains_create(self.chainset), "approx": lambda: p.approx_create(self.approxset),
                                    "edit": lambda: p.approx_create(self.approxset), "templates": lambda: p.templates_create(self.templateset),
                                    "flows": lambda: binding.Flows(p, self.T)}[family]()
        return self.handles[family]

    # -- what the cases share
    def _text(self):
        return {"text": (self.real, self.decoy)}

    def _records(self, sel=False):
        """the gated text, records (oracle's, cut to one number, in a room of CAP) and their count on the device"""
        r, d, n = (self.sel, self.sel_decoy, self.ns) if sel else (self.rec, self.rec_decoy, self.n)
        return {"text": (self.real, self.decoy), "rec": (padded(r[:n], CAP), padded(d[:n], CAP)),
                "n": (np.array([n], np.uint64), np.array([n], np.uint64))}, n

    def case(self, name):
        return getattr(self, "_" + name[len("acm_gpu_"):])(name)

    # -- what every entry point must give, without the library's scans, joins and host passes
    def expected(self, name, which="real"):
        """the expected value of every output of case (name) that has a definition (None: one that has none), for the real
        or the decoy inputs: the oracle's records and the definitions of tests/*_cases.py"""
        if (name, which) not in self.wants:
            self.wants[(name, which)] = [None if w is None else np.asarray(w) for w in getattr(self, "_want_" + name[len("acm_gpu_"):])(which)]
        return self.wants[(name, which)]

    def _side(self, which):
        """(text, the batch's records, the selection of them, the records of the buffer as one text)"""
        assert which in ("real", "decoy")
        real = which == "real"
        return (self.real if real else self.decoy, self.rec if real else self.rec_decoy, self.sel if real else self.sel_decoy, self.whole[which])

    def _texts(self, text):
        return [text[int(self.off[t]):int(self.off[t + 1])] for t in range(self.T)]

    def _want_scan_batch_device(self, which):
        _, rec, _, _ = self._side(which)
        return [rec_rows(rec), self._text_ids(rec), self._first(rec), [rec.size]]

    def _want_flow(self, steps):
        rec, tid, first = flow_cases.expected(self.o, steps)[-1]
        return [rec_rows(rec), i32(tid), i64(first), [rec.size]]

    def _want_scan_flows_device(self, which):
        flows = range(self.T)
        return self._want_flow([flow_cases.Call(self._texts(self.pre_text), flows), flow_cases.Call(self._texts(self._side(which)[0]), flows)])

    def _want_flows_reset(self, which):
        flows = range(self.T)
        ids = range(0 if which == "real" else 1, 2 * (self.T // 2), 2)
        return self._want_flow([flow_cases.Call(self._texts(self.pre_text), flows), flow_cases.Reset(ids), flow_cases.Call(self._texts(self.real), flows)])

    def _want_tally_device(self, which):
        whole = self._side(which)[3]
        return [np.bincount(whole["keyword_id"], minlength=self.K).astype(np.int64), [whole.size]]

    def _want_grep_device(self, which):
        text, rec, _, _ = self._side(which)
        hits = np.diff(self._first(rec)).astype(np.uint64)
        kept, out_off, out = grep_cases.expected(text, self.off, hits, False)
        return [i64(hits), i32(kept), None, out, i64(out_off), [kept.size, int(hits.sum()), out.size]]

    def _want_tally_batch_device(self, which):
        rec = self._side(which)[1]
        matrix = self._matrix(rec)
        return matrix + [None, [matrix[1].size, rec.size]]

    def _counts(self, rec):
        rp, c, v = self._matrix(rec)
        return rp.astype(np.uint64), c.astype(np.uint32), v.astype(np.uint64)

    def _want_rules_matrix_device(self, which):
        fired_ptr, fired, _ = rules_cases.expected_fired(self._counts(self._side(which)[1]), self.K, self.ruleset)
        return [i64(fired_ptr), i32(fired), [fired.size]]

    def _want_rules_device(self, which):
        rec = self._side(which)[1]
        fired_ptr, fired, _ = rules_cases.expected_fired(self._counts(rec), self.K, self.ruleset)
        return [i64(fired_ptr), i32(fired), None, [fired.size, rec.size]]

    def _want_split_device(self, which):
        off = split_cases.expected_offsets(self._side(which)[0], self.delim, runs=False)
        return [i64(off), [off.size - 1]]

    def _want_select_records_device(self, which):
        sel = greedy(self._side(which)[1][:self.n])
        return [rec_rows(sel), [sel.size]]

    def _want_scan_select_device(self, which):
        sel = greedy(self._side(which)[3])
        return [rec_rows(sel), [sel.size]]

    def _want_replace_records_device(self, which):
        text, _, sel, _ = self._side(which)
        out, starts = replace_cases.replace_by_definition(text, sel[:self.ns], self.repl)
        return [out, [out.size], starts]

    def _want_scan_replace_device(self, which):
        text, _, _, whole = self._side(which)
        sel = greedy(whole)
        out, starts = replace_cases.replace_by_definition(text, sel, self.repl)
        return [rec_rows(sel), [sel.size], out, [out.size], starts]

    def _want_tokens(self, text, sel):
        ids, starts, lens, first = token_cases.tokens_by_definition(text, sel, token_cases.RUN, gap_base=1000, offsets=self.off)
        return [i32(ids), i64(starts), i32(lens), [ids.size], i64(first)]

    def _want_tokens_records_device(self, which):
        text, _, sel, _ = self._side(which)
        return self._want_tokens(text, sel[:self.ns])

    def _want_scan_tokens_device(self, which):
        text, rec, _, _ = self._side(which)
        sel = greedy(rec)                                # (a batch's records never cross a text: one selection serves all texts)
        return [rec_rows(sel), [sel.size]] + self._want_tokens(text, sel)

    def _want_words(self, text, rec):
        w = words_cases.words(rec, text, self.off, self.word_ranges, words_cases.BOTH)
        return [rec_rows(w), [w.size]]

    def _want_words_records_device(self, which):
        text, rec, _, _ = self._side(which)
        return self._want_words(text, rec[:self.n])

    def _want_scan_words_device(self, which):
        text, _, _, whole = self._side(which)
        return self._want_words(text, whole)

    def _want_context(self, text, rec):
        e = context_cases.expected(rec, self.N, self.off, before=3, after=2, texts=False, merged=True)
        return [e.out(text), [e.out_symbols], [e.n_snippets], i64(e.snip_lo), i64(e.out_offsets), i32(e.snip_text), i32(e.rec_snip), e.rec_at]

    def _want_context_records_device(self, which):
        text, rec, _, _ = self._side(which)
        return self._want_context(text, rec[:self.n])

    def _want_scan_context_device(self, which):
        text, _, _, whole = self._side(which)
        return [rec_rows(whole), [whole.size]] + self._want_context(text, whole)

    def _want_join(self, which, fused, definition):
        """a join of the batch's first n records, or (fused) of the records of the buffer as one text; definition
        (records, text) gives the matches, or (matches, distances)"""
        text, rec, _, whole = self._side(which)
        got = definition(whole if fused else rec[:self.n], text)
        got = list(got) if isinstance(got, tuple) else [got]
        return [rec_rows(got[0])] + [i32(d) for d in got[1:]] + [[got[0].size, whole.size] if fused else [got[0].size]]

    def _patterns_by_definition(self, rec, text):
        return pattern_cases.patterns(rec, terms_of(self.patternset.terms, self.patternset.pat_ptr), self.N, self.off)

    def _chains_by_definition(self, rec, text):
        return chain_cases.chains(rec, chain_cases.chain_terms(self.chainset), self.N, self.off)

    def _approx_by_definition(self, rec, text):
        return approx_cases.approx(rec, text, self.targets, self.target_k, terms_of(self.approxset.terms, self.approxset.tgt_ptr), self.off)

    def _edit_by_definition(self, rec, text):
        return edit_cases.edits(rec, text, self.targets, self.target_k, terms_of(self.approxset.terms, self.approxset.tgt_ptr), self.off)

    def _templates_by_definition(self, rec, text):
        return template_cases.templates(rec, text, self.templates, self.template_k, terms_of(self.templateset.terms, self.templateset.tgt_ptr), self.off)

    def _want_patterns_records_device(self, which):
        return self._want_join(which, False, self._patterns_by_definition)

    def _want_scan_patterns_device(self, which):
        return self._want_join(which, True, self._patterns_by_definition)

    def _want_chains_records_device(self, which):
        return self._want_join(which, False, self._chains_by_definition)

    def _want_scan_chains_device(self, which):
        return self._want_join(which, True, self._chains_by_definition)

    def _want_approx_records_device(self, which):
        return self._want_join(which, False, self._approx_by_definition)

    def _want_scan_approx_device(self, which):
        return self._want_join(which, True, self._approx_by_definition)

    def _want_edit_records_device(self, which):
        return self._want_join(which, False, self._edit_by_definition)

    def _want_scan_edit_device(self, which):
        return self._want_join(which, True, self._edit_by_definition)

    def _want_templates_records_device(self, which):
        return self._want_join(which, False, self._templates_by_definition)

    def _want_scan_templates_device(self, which):
        return self._want_join(which, True, self._templates_by_definition)

    # -- batch and flows
    def _scan_batch_device(self, name):
        import torch as T
        L, h, N, Tn, off = binding.lib(), self.plan.h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_scan_batch_tmp_bytes(h, CAP, N, Tn)
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_scan_batch_device(h, p["text"], N, off, Tn, p["rec"], p["tid"], p["first"], CAP, p["count"], p["tmp"], tb, st),
                    self._text(), {"rec": (2 * CAP, T.int64), "tid": (CAP, T.int32), "first": (Tn + 1, T.int64), "count": (1, T.int64)}, tb,
                    cut=lambda x: [rows(x, "rec", x["count"][0]), x["tid"][:x["count"][0]], x["first"], x["count"]],
                    want=self.expected(name))

    def _text_ids(self, rec):
        """(the last text that begins at or before end_pos: the one that is not empty)"""
        return (np.searchsorted(self.off, rec["end_pos"], side="right") - 1).astype(np.int32)

    def _first(self, rec):
        tid = self._text_ids(rec)
        return np.concatenate(([0], np.cumsum(np.bincount(tid, minlength=self.T)))).astype(np.int64)

    def _flows_pre(self):
        """the piece every flow is fed before the gated call: the decoy text shifted, so that carries are in place"""
        torch = self.torch
        if not hasattr(self, "pre"):
            import torch as T
            L, h, fh = binding.lib(), self.plan.h, self.handle("flows").h
            tb = L.acm_gpu_scan_flows_tmp_bytes(h, fh, CAP, self.N, self.T)
            self.pre = dict(text=dev(torch, self.pre_text), rec=T.zeros(2 * CAP, dtype=T.int64, device="cuda"),
                            count=T.zeros(1, dtype=T.int64, device="cuda"), tmp=T.zeros(max(tb, 16), dtype=T.uint8, device="cuda"), tb=tb)
        return self.pre

    def _feed_pre(self, p):
        """all flows back to the root, then the first piece, on the null stream, synchronised"""
        L, h, fh, pre = binding.lib(), self.plan.h, self.handle("flows").h, self._flows_pre()
        assert L.acm_gpu_flows_reset(fh, None, 0, None) == OK
        assert L.acm_gpu_scan_flows_device(h, fh, pre["text"].data_ptr(), self.N, self.d_off.data_ptr(), None, self.T, pre["rec"].data_ptr(), None, None,
                                           CAP, pre["count"].data_ptr(), pre["tmp"].data_ptr(), pre["tb"], None) == OK
        self.torch.cuda.synchronize()
        assert 0 < int(pre["count"].item()) <= CAP

    def _scan_flows_device(self, name):
        import torch as T
        L, h, fh, N, Tn, off = binding.lib(), self.plan.h, self.handle("flows").h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_scan_flows_tmp_bytes(h, fh, CAP, N, Tn)
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_scan_flows_device(h, fh, p["text"], N, off, None, Tn, p["rec"], p["tid"], p["first"], CAP, p["count"], p["tmp"],
                                                              tb, st),
                    self._text(), {"rec": (2 * CAP, T.int64), "tid": (CAP, T.int32), "first": (Tn + 1, T.int64), "count": (1, T.int64)}, tb,
                    cut=lambda x: [rows(x, "rec", x["count"][0]), x["tid"][:x["count"][0]], x["first"], x["count"]], prepare=self._feed_pre,
                    want=self.expected(name))

    def _flows_reset(self, name):
        """flows reset on the stream, seen by a flow scan of the real text behind it: the real ids are the even flows,
        the decoy's the odd ones"""
        import torch as T
        L, h, fh, N, Tn, off = binding.lib(), self.plan.h, self.handle("flows").h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_scan_flows_tmp_bytes(h, fh, CAP, N, Tn)
        k = Tn // 2
        ids = {"ids": (np.arange(0, 2 * k, 2, dtype=np.uint32), np.arange(1, 2 * k, 2, dtype=np.uint32))}
        d_text = dev(self.torch, self.real)
        self.keep.append(d_text)

        def post(p, st):
            assert L.acm_gpu_scan_flows_device(h, fh, d_text.data_ptr(), N, off, None, Tn, p["rec"], p["tid"], p["first"], CAP, p["count"], p["tmp"], tb,
                                               st) == OK
        return Case(name, self.plan, lambda p, st: L.acm_gpu_flows_reset(fh, p["ids"], k, st), ids,
                    {"rec": (2 * CAP, T.int64), "tid": (CAP, T.int32), "first": (Tn + 1, T.int64), "count": (1, T.int64)}, tb,
                    cut=lambda x: [rows(x, "rec", x["count"][0]), x["tid"][:x["count"][0]], x["first"], x["count"]], prepare=self._feed_pre, post=post,
                    want=self.expected(name))

    # -- tallies, grep, rules, split
    def _tally_device(self, name):
        import torch as T
        L, h, N, K = binding.lib(), self.plan.h, self.N, self.K
        tb = L.acm_gpu_tally_tmp_bytes(h, WINDOW, CAP)
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_tally_device(h, p["text"], N, 0, p["tally"], K, WINDOW, CAP, p["res"], p["res"] + 8, p["tmp"], tb, st),
                    self._text(), {"tally": (K, T.int64), "res": (2, T.int64)}, tb, accumulate=("tally",),
                    cut=lambda x: [x["tally"], x["res"][:1]], want=self.expected(name))

    def _grep_device(self, name):
        import torch as T
        L, h, N, Tn, off = binding.lib(), self.plan.h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_grep_tmp_bytes(h, WINDOW, CAP, N, Tn)

        def cut(x):
            n_kept, _, _, out_symbols = (int(v) for v in x["res"])
            return [x["hits"], x["kept"][:n_kept], x["res"], x["out"][:out_symbols], x["out_off"][:n_kept + 1], x["res"][[0, 1, 3]]]
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_grep_device(h, p["text"], N, off, Tn, binding.ACM_GREP_MATCHING, WINDOW, CAP, p["hits"], p["kept"], p["res"],
                                                        p["res"] + 8, p["res"] + 16, p["out"], N, p["out_off"], p["res"] + 24, p["tmp"], tb, st),
                    self._text(), {"hits": (Tn, T.int64), "kept": (Tn, T.int32), "res": (4, T.int64), "out": (N, T.uint8), "out_off": (Tn + 1, T.int64)},
                    tb, cut=cut, want=self.expected(name))

    def _tally_batch_device(self, name):
        import torch as T
        L, h, N, Tn, off = binding.lib(), self.plan.h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_tally_batch_tmp_bytes(h, WINDOW, CAP, CAP, N, Tn)
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_tally_batch_device(h, p["text"], N, off, Tn, WINDOW, CAP, CAP, p["row_ptr"], p["col"], p["val"], p["res"],
                                                               p["res"] + 8, p["res"] + 16, p["res"] + 24, p["tmp"], tb, st),
                    self._text(), {"row_ptr": (Tn + 1, T.int64), "col": (CAP, T.int32), "val": (CAP, T.int64), "res": (4, T.int64)}, tb,
                    cut=lambda x: [x["row_ptr"], x["col"][:x["res"][0]], x["val"][:x["res"][0]], x["res"], x["res"][:2]], want=self.expected(name))

    def _matrix(self, rec):
        """the text x keyword count matrix of batch records in CSR form, columns ascending: [row_ptr, col, val]"""
        tid = self._text_ids(rec)
        row_ptr, col, val = [0], [], []
        for t in range(self.T):
            ids, counts = np.unique(rec["keyword_id"][tid == t], return_counts=True)
            col += [int(i) for i in ids]
            val += [int(c) for c in counts]
            row_ptr.append(len(col))
        return [np.array(row_ptr, np.int64), np.array(col, np.int32), np.array(val, np.int64)]

    def _rules_matrix_device(self, name):
        import torch as T
        L, h, R, Tn = binding.lib(), self.plan.h, self.handle("rules").h, self.T
        tb = L.acm_gpu_rules_matrix_tmp_bytes(h, R, Tn)
        FC = Tn * self.ruleset.n_rules
        (rp, c, v), (rp2, c2, v2) = self._matrix(self.rec), self._matrix(self.rec_decoy)
        room = max(c.size, c2.size)

        def pad(a):
            return np.concatenate([a, np.zeros(room - a.size, a.dtype)])
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_rules_matrix_device(h, R, p["row_ptr"], p["col"], p["val"], Tn, p["fired_ptr"], p["fired"], FC, p["n_fired"],
                                                                p["tmp"], tb, st),
                    {"row_ptr": (rp, rp2), "col": (pad(c), pad(c2)), "val": (pad(v), pad(v2))},
                    {"fired_ptr": (Tn + 1, T.int64), "fired": (FC, T.int32), "n_fired": (1, T.int64)}, tb,
                    cut=lambda x: [x["fired_ptr"], x["fired"][:x["n_fired"][0]], x["n_fired"]], want=self.expected(name))

    def _rules_device(self, name):
        import torch as T
        L, h, R, N, Tn, off = binding.lib(), self.plan.h, self.handle("rules").h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_rules_tmp_bytes(h, R, WINDOW, CAP, CAP, N, Tn)
        FC = Tn * self.ruleset.n_rules
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_rules_device(h, R, p["text"], N, off, Tn, WINDOW, CAP, CAP, p["fired_ptr"], p["fired"], FC, p["res"], p["res"] + 8,
                                                         p["res"] + 16, p["res"] + 24, p["tmp"], tb, st),
                    self._text(), {"fired_ptr": (Tn + 1, T.int64), "fired": (FC, T.int32), "res": (4, T.int64)}, tb,
                    cut=lambda x: [x["fired_ptr"], x["fired"][:x["res"][0]], x["res"], x["res"][:2]], want=self.expected(name))

    def _split_device(self, name):
        import torch as T
        L, h, N = binding.lib(), self.plan.h, self.N
        tb = L.acm_gpu_split_tmp_bytes(h, N)
        d, nd = self.delims, self.n_delims
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_split_device(h, p["text"], N, d.ctypes.data, nd, binding.ACM_SPLIT_EVERY, p["off"], N, p["count"], p["tmp"], tb, st),
                    self._text(), {"off": (N + 1, T.int64), "count": (1, T.int64)}, tb,
                    cut=lambda x: [x["off"][:x["count"][0] + 1], x["count"]], want=self.expected(name))

    # -- select, replace, tokens, words, context
    def _select_records_device(self, name):
        import torch as T
        L, h, N = binding.lib(), self.plan.h, self.N
        tb = L.acm_gpu_select_tmp_bytes(h, CAP, N)
        gated, _ = self._records()
        del gated["text"]
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_select_records_device(h, p["rec"], CAP, p["n"], 0, N, p["out"], p["count"], p["tmp"], tb, st),
                    gated, {"out": (2 * CAP, T.int64), "count": (1, T.int64)}, tb,
                    cut=lambda x: [rows(x, "out", x["count"][0]), x["count"]], want=self.expected(name))

    def _scan_select_device(self, name):
        import torch as T
        L, h, N = binding.lib(), self.plan.h, self.N
        tb = L.acm_gpu_scan_select_tmp_bytes(h, CAP, N)
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_scan_select_device(h, p["text"], N, 0, p["rec"], CAP, p["count"], p["tmp"], tb, st),
                    self._text(), {"rec": (2 * CAP, T.int64), "count": (1, T.int64)}, tb,
                    cut=lambda x: [rows(x, "rec", x["count"][0]), x["count"]], want=self.expected(name))

    def _replace_outs(self):
        import torch as T
        return {"out": (4 * self.N, T.uint8), "out_symbols": (1, T.int64), "out_start": (CAP, T.int64)}

    def _replace_records_device(self, name):
        L, h, N, K = binding.lib(), self.plan.h, self.N, self.K
        tb = L.acm_gpu_replace_tmp_bytes(h, CAP, N)
        gated, n = self._records(sel=True)
        rd, ro = self.d_repl.data_ptr(), self.d_repl_off.data_ptr()
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_replace_records_device(h, p["text"], N, 0, p["rec"], CAP, p["n"], rd, ro, K, p["out"], 4 * N, p["out_symbols"],
                                                                   p["out_start"], p["tmp"], tb, st),
                    gated, self._replace_outs(), tb,
                    cut=lambda x: [x["out"][:self._inside(x["out_symbols"][0], 4 * N)], x["out_symbols"], x["out_start"][:n]], want=self.expected(name))

    def _scan_replace_device(self, name):
        import torch as T
        L, h, N, K = binding.lib(), self.plan.h, self.N, self.K
        tb = L.acm_gpu_scan_replace_tmp_bytes(h, CAP, N)
        rd, ro = self.d_repl.data_ptr(), self.d_repl_off.data_ptr()
        outs = dict(self._replace_outs(), rec=(2 * CAP, T.int64), count=(1, T.int64))
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_scan_replace_device(h, p["text"], N, 0, p["rec"], CAP, p["count"], rd, ro, K, p["out"], 4 * N, p["out_symbols"],
                                                                p["out_start"], p["tmp"], tb, st),
                    self._text(), outs, tb,
                    cut=lambda x: [rows(x, "rec", x["count"][0]), x["count"], x["out"][:self._inside(x["out_symbols"][0], 4 * N)],
                                   x["out_symbols"], x["out_start"][:x["count"][0]]], want=self.expected(name))

    def _token_outs(self):
        import torch as T
        return {"tok_id": (self.N, T.int32), "tok_start": (self.N, T.int64), "tok_len": (self.N, T.int32), "n_tokens": (1, T.int64),
                "tok_first": (self.T + 1, T.int64)}

    @staticmethod
    def _token_cut(x):
        n = int(x["n_tokens"][0])
        return [x["tok_id"][:n], x["tok_start"][:n], x["tok_len"][:n], x["n_tokens"], x["tok_first"]]

    def _tokens_records_device(self, name):
        L, h, N, Tn, K, off = binding.lib(), self.plan.h, self.N, self.T, self.K, self.d_off.data_ptr()
        tb = L.acm_gpu_tokens_tmp_bytes(h, CAP, N)
        gated, n = self._records(sel=True)
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_tokens_records_device(h, p["text"], N, 0, p["rec"], CAP, p["n"], off, Tn, None, K, 1000, binding.TOKENS_GAP_RUN,
                                                                  p["tok_id"], p["tok_start"], p["tok_len"], N, p["n_tokens"], p["tok_first"], p["tmp"], tb, st),
                    gated, self._token_outs(), tb, cut=self._token_cut, want=self.expected(name))

    def _scan_tokens_device(self, name):
        import torch as T
        L, h, N, Tn, K, off = binding.lib(), self.plan.h, self.N, self.T, self.K, self.d_off.data_ptr()
        tb = L.acm_gpu_scan_tokens_tmp_bytes(h, CAP, N, Tn)
        outs = dict(self._token_outs(), rec=(2 * CAP, T.int64), count=(1, T.int64))
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_scan_tokens_device(h, p["text"], N, 0, off, Tn, p["rec"], CAP, p["count"], None, K, 1000, binding.TOKENS_GAP_RUN,
                                                               p["tok_id"], p["tok_start"], p["tok_len"], N, p["n_tokens"], p["tok_first"], p["tmp"], tb, st),
                    self._text(), outs, tb, cut=lambda x: [rows(x, "rec", x["count"][0]), x["count"]] + self._token_cut(x), want=self.expected(name))

    def _words_records_device(self, name):
        import torch as T
        L, h, N, Tn, off = binding.lib(), self.plan.h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_words_tmp_bytes(h, CAP, Tn)
        gated, n = self._records()
        r, nr = self.ranges, self.n_ranges
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_words_records_device(h, p["text"], N, 0, off, Tn, r.ctypes.data, nr, binding.ACM_WORDS_BOTH, p["rec"], CAP, p["n"],
                                                                 p["out"], p["count"], p["tmp"], tb, st),
                    gated, {"out": (2 * CAP, T.int64), "count": (1, T.int64)}, tb, cut=lambda x: [rows(x, "out", x["count"][0]), x["count"]],
                    want=self.expected(name))

    def _scan_words_device(self, name):
        import torch as T
        L, h, N, Tn, off = binding.lib(), self.plan.h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_scan_words_tmp_bytes(h, CAP, N, Tn)
        r, nr = self.ranges, self.n_ranges
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_scan_words_device(h, p["text"], N, 0, off, Tn, r.ctypes.data, nr, binding.ACM_WORDS_BOTH, p["rec"], CAP,
                                                              p["count"], p["tmp"], tb, st),
                    self._text(), {"rec": (2 * CAP, T.int64), "count": (1, T.int64)}, tb, cut=lambda x: [rows(x, "rec", x["count"][0]), x["count"]],
                    want=self.expected(name))

    def _context_outs(self):
        import torch as T
        return {"out": (8 * self.N, T.uint8), "out_symbols": (1, T.int64), "n_snippets": (1, T.int64), "snip_lo": (CAP, T.int64),
                "out_off": (CAP + 1, T.int64), "snip_text": (CAP, T.int32), "rec_snip": (CAP, T.int32), "rec_at": (CAP, T.int64)}

    @staticmethod
    def _inside(n, capacity):
        assert 0 <= int(n) <= capacity, (int(n), capacity)
        return int(n)

    def _context_cut(self, x, n):
        s = int(x["n_snippets"][0])
        return [x["out"][:self._inside(x["out_symbols"][0], 8 * self.N)], x["out_symbols"], x["n_snippets"], x["snip_lo"][:s], x["out_off"][:s + 1],
                x["snip_text"][:s], x["rec_snip"][:n], x["rec_at"][:n]]

    def _context_records_device(self, name):
        L, h, N, Tn, off = binding.lib(), self.plan.h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_context_tmp_bytes(h, CAP, Tn)
        gated, n = self._records()
        flags = binding.ACM_CONTEXT_SYMBOLS | binding.ACM_CONTEXT_MERGE
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_context_records_device(h, p["text"], N, 0, off, Tn, p["rec"], CAP, p["n"], 3, 2, flags, p["out"], 8 * N,
                                                                   p["out_symbols"], p["n_snippets"], p["snip_lo"], p["out_off"], p["snip_text"],
                                                                   p["rec_snip"], p["rec_at"], p["tmp"], tb, st),
                    gated, self._context_outs(), tb, cut=lambda x: self._context_cut(x, n), want=self.expected(name))

    def _scan_context_device(self, name):
        import torch as T
        L, h, N, Tn, off = binding.lib(), self.plan.h, self.N, self.T, self.d_off.data_ptr()
        tb = L.acm_gpu_scan_context_tmp_bytes(h, CAP, N, Tn)
        flags = binding.ACM_CONTEXT_SYMBOLS | binding.ACM_CONTEXT_MERGE
        outs = dict(self._context_outs(), rec=(2 * CAP, T.int64), count=(1, T.int64))
        return Case(name, self.plan,
                    lambda p, st: L.acm_gpu_scan_context_device(h, p["text"], N, 0, off, Tn, p["rec"], CAP, p["count"], 3, 2, flags, p["out"], 8 * N,
                                                                p["out_symbols"], p["n_snippets"], p["snip_lo"], p["out_off"], p["snip_text"],
                                                                p["rec_snip"], p["rec_at"], p["tmp"], tb, st),
                    self._text(), outs, tb, cut=lambda x: [rows(x, "rec", x["count"][0]), x["count"]] + self._context_cut(x, int(x["count"][0])),
                    want=self.expected(name))

    # -- the set families: patterns and chains (records in, records out), approx, edit and templates (with distances)
    def _join_records(self, name, family, most):
        import torch as T
        L, h, S, N, Tn, off = binding.lib(), self.plan.h, self.handle(family).h, self.N, self.T, self.d_off.data_ptr()
        OC = CAP * most
        tb = getattr(L, "acm_gpu_%s_tmp_bytes" % family)(h, S, CAP, Tn)
        gated, n = self._records()
        del gated["text"]
        return Case(name, self.plan,
                    lambda p, st: getattr(L, name)(h, S, p["rec"], CAP, p["n"], N, 0, off, Tn, p["out"], OC, p["count"], p["tmp"], tb, st),
                    gated, {"out": (2 * OC, T.int64), "count": (1, T.int64)}, tb, cut=lambda x: [rows(x, "out", x["count"][0]), x["count"]],
                    want=self.expected(name) if hasattr(self, "_want_" + name[len("acm_gpu_"):]) else None)

    def _join_scan(self, name, family, most):
        import torch as T
        L, h, S, N, Tn, off = binding.lib(), self.plan.h, self.handle(family).h, self.N, self.T, self.d_off.data_ptr()
        OC = CAP * most
        tb = getattr(L, "acm_gpu_scan_%s_tmp_bytes" % family)(h, S, CAP, N, Tn)
        return Case(name, self.plan,
                    lambda p, st: getattr(L, name)(h, S, p["text"], N, 0, off, Tn, CAP, p["out"], OC, p["res"], p["res"] + 8, p["tmp"], tb, st),
                    self._text(), {"out": (2 * OC, T.int64), "res": (2, T.int64)}, tb, cut=lambda x: [rows(x, "out", x["res"][0]), x["res"]],
                    want=self.expected(name) if hasattr(self, "_want_" + name[len("acm_gpu_"):]) else None)

    def _patterns_records_device(self, name):
        return self._join_records(name, "patterns", int(self.handle("patterns").info()["max_anchor_postings"]))

    def _scan_patterns_device(self, name):
        return self._join_scan(name, "patterns", int(self.handle("patterns").info()["max_anchor_postings"]))

    def _chains_records_device(self, name):
        return self._join_records(name, "chains", int(self.handle("chains").info()["max_last_postings"]))

    def _scan_chains_device(self, name):
        return self._join_scan(name, "chains", int(self.handle("chains").info()["max_last_postings"]))

    def _most(self, family):
        return self.plan._most_per_record("edit" if family == "edit" else "approx", self.handle(family).info())

    def _verify_records(self, name, family):
        import torch as T
        L, h, S, N, Tn, off = binding.lib(), self.plan.h, self.handle(family).h, self.N, self.T, self.d_off.data_ptr()
        OC = CAP * self._most(family)
        tb = getattr(L, "acm_gpu_%s_tmp_bytes" % family)(h, S, CAP, OC, Tn)
        gated, n = self._records()
        return Case(name, self.plan,
                    lambda p, st: getattr(L, name)(h, S, p["rec"], CAP, p["n"], p["text"], N, 0, off, Tn, p["out"], p["dist"], OC, p["count"], p["tmp"], tb,
                                                   st),
                    gated, {"out": (2 * OC, T.int64), "dist": (OC, T.int32), "count": (1, T.int64)}, tb,
                    cut=lambda x: [rows(x, "out", x["count"][0]), x["dist"][:x["count"][0]], x["count"]], want=self.expected(name))

    def _verify_scan(self, name, family):
        import torch as T
        L, h, S, N, Tn, off = binding.lib(), self.plan.h, self.handle(family).h, self.N, self.T, self.d_off.data_ptr()
        OC = CAP * self._most(family)
        tb = getattr(L, "acm_gpu_scan_%s_tmp_bytes" % family)(h, S, CAP, OC, N, Tn)
        return Case(name, self.plan,
                    lambda p, st: getattr(L, name)(h, S, p["text"], N, 0, off, Tn, CAP, p["out"], p["dist"], OC, p["res"], p["res"] + 8, p["tmp"], tb, st),
                    self._text(), {"out": (2 * OC, T.int64), "dist": (OC, T.int32), "res": (2, T.int64)}, tb,
                    cut=lambda x: [rows(x, "out", x["res"][0]), x["dist"][:x["res"][0]], x["res"]], want=self.expected(name))

    def _approx_records_device(self, name):
        return self._verify_records(name, "approx")

    def _scan_approx_device(self, name):
        return self._verify_scan(name, "approx")

    def _edit_records_device(self, name):
        return self._verify_records(name, "edit")

    def _scan_edit_device(self, name):
        return self._verify_scan(name, "edit")

    def _templates_records_device(self, name):
        return self._verify_records(name, "templates")

    def _scan_templates_device(self, name):
        return self._verify_scan(name, "templates")


FEATURES = ["acm_gpu_scan_batch_device", "acm_gpu_flows_reset", "acm_gpu_scan_flows_device",
            "acm_gpu_tally_device", "acm_gpu_grep_device", "acm_gpu_tally_batch_device", "acm_gpu_rules_matrix_device", "acm_gpu_rules_device",
            "acm_gpu_split_device",
            "acm_gpu_select_records_device", "acm_gpu_scan_select_device",
            "acm_gpu_replace_records_device", "acm_gpu_scan_replace_device",
            "acm_gpu_tokens_records_device", "acm_gpu_scan_tokens_device",
            "acm_gpu_words_records_device", "acm_gpu_scan_words_device",
            "acm_gpu_context_records_device", "acm_gpu_scan_context_device",
            "acm_gpu_patterns_records_device", "acm_gpu_scan_patterns_device",
            "acm_gpu_approx_records_device", "acm_gpu_scan_approx_device",
            "acm_gpu_edit_records_device", "acm_gpu_scan_edit_device",
            "acm_gpu_chains_records_device", "acm_gpu_scan_chains_device",
            "acm_gpu_templates_records_device", "acm_gpu_scan_templates_device"]
ANCHORED = ["acm_gpu_scan_anchored_device", "acm_gpu_lookup_device"]
TOOLING = ["acm_gpu_synth_text"]
# the fused forms: a scan with passes behind it in one call -- run a second time on the 4-gram kind
FUSED = [f for f in FEATURES if "_scan_" in f]
# one control per feature family (the plain scans have one per plan kind)
CONTROLS = ["acm_gpu_scan_batch_device", "acm_gpu_flows_reset", "acm_gpu_tally_device", "acm_gpu_grep_device", "acm_gpu_tally_batch_device",
            "acm_gpu_rules_device", "acm_gpu_split_device", "acm_gpu_scan_select_device", "acm_gpu_scan_replace_device", "acm_gpu_scan_tokens_device",
            "acm_gpu_scan_words_device", "acm_gpu_scan_context_device", "acm_gpu_scan_anchored_device", "acm_gpu_scan_patterns_device",
            "acm_gpu_scan_approx_device", "acm_gpu_scan_edit_device", "acm_gpu_scan_chains_device", "acm_gpu_scan_templates_device",
            "acm_gpu_synth_text"]
# the table the completeness guard reads: every entry point that has a stream case
CASES = PLAIN + FEATURES + ANCHORED + TOOLING


def anchored_cases(torch, plan, real, decoy, off):
    """acm_gpu_scan_anchored_device and acm_gpu_lookup_device on the anchored tests' own small batch"""
    import torch as T
    L, h, N, Tn = binding.lib(), plan.h, real.size, off.size - 1
    d_off = dev(torch, off)
    o_ptr = d_off.data_ptr()
    cap = 8 * Tn
    tba, tbl = L.acm_gpu_scan_anchored_tmp_bytes(h, Tn), L.acm_gpu_lookup_tmp_bytes(h, Tn)
    text = {"text": (real, decoy)}
    return [Case("acm_gpu_scan_anchored_device", plan,
                 lambda p, st: L.acm_gpu_scan_anchored_device(h, p["text"], N, o_ptr, Tn, binding.ACM_ANCHORED_PREFIXES, p["rec"], p["tid"], p["first"], cap,
                                                              p["count"], p["tmp"], tba, st),
                 text, {"rec": (2 * cap, T.int64), "tid": (cap, T.int32), "first": (Tn + 1, T.int64), "count": (1, T.int64)}, tba,
                 cut=lambda x: [rows(x, "rec", x["count"][0]), x["tid"][:x["count"][0]], x["first"], x["count"]], keep=d_off),
            Case("acm_gpu_lookup_device", plan,
                 lambda p, st: L.acm_gpu_lookup_device(h, p["text"], N, o_ptr, Tn, p["whole"], p["prefix"], p["length"], p["tmp"], tbl, st),
                 text, {"whole": (Tn, T.int32), "prefix": (Tn, T.int32), "length": (Tn, T.int32)}, tbl, keep=d_off)]


def synth_case(torch, plan, kw_data, kw_off, n=1 << 16):
    """acm_gpu_synth_text: the keywords it plants are the gated input (the decoy: the same keywords spelt backwards)"""
    import torch as T
    L = binding.lib()
    kd = np.ascontiguousarray(kw_data, dtype=np.uint8)
    ko = np.ascontiguousarray(kw_off, dtype=np.uint32)
    d_off = dev(torch, ko)
    o_ptr, K = d_off.data_ptr(), ko.size - 1
    return Case("acm_gpu_synth_text", plan, lambda p, st: L.acm_gpu_synth_text(0, p["text"], n, 0, 1, 0, p["kw"], o_ptr, K, st),
                {"kw": (kd, kd[::-1].copy())}, {"text": (n, T.uint8)}, keep=d_off)
