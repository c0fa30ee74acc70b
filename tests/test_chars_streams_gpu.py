"""The four device entry points of include/acm_chars.h on a stream that is not the default one: the EARLY / LATE /
CONTROL arrangements of tests/stream_cases.py (Gates, Case, exercise) over two valid UTF-8 texts of one length under one
offsets[].  The ruler pass, its two prefix sums, the memset of a map's control word, the check of offsets[], the maps and
the ordered scan in front of the fused call all have to be queued on the caller's stream.  A ruler has no definition of
its own: its case reads it back through the positions call, every rank of the text.  The expected value is the
definition in numpy (tests/chars_cases.py) over the oracle's records, never the library's own scan."""
import ctypes as C
import os

import numpy as np
import pytest

from aho_corasick_1975_amd import binding
from tests import chars_cases as cc
from tests import stream_cases as sc
from tests.cases import build_pair

HEADER = os.path.join(sc.ROOT, "include", "acm_chars.h")
ENTRIES = ["acm_gpu_chars_ruler_device", "acm_gpu_chars_records_device", "acm_gpu_chars_positions_device", "acm_gpu_scan_chars_device"]
N, CAP = 4096, 4096
UNIT = cc.UTF16


def test_every_stream_entry_point_of_the_header_is_exercised():
    assert sorted(sc.header_stream_functions(path=HEADER)) == sorted(ENTRIES)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


class _Gates(sc.Gates):
    """stream_cases.Gates over a side stream that is handed in: the same calibration of torch.cuda._sleep"""

    def __init__(self, torch, side):
        self.torch, self.side = torch, side
        assert side.cuda_stream != 0 and torch.cuda.default_stream().cuda_stream == 0
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
        self.longest_plain_ms = self.longest_gate_ms = 0.0


def _hip_runtime():
    """the HIP runtime this process has loaded, as a ctypes library"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


@pytest.fixture(scope="module")
def gates(torch_cuda):
    """A stream takes one of the process's few hardware queues, the least loaded one, and torch never gives a stream of
    its pool back: one more pool stream here would move the side stream of every module behind this one to another queue,
    onto the null stream's for some -- where a gate holds the null stream up and a CONTROL run cannot tell the two apart.
    So the side stream of this module is a HIP stream of its own that is destroyed with the module: four are made, the
    first that demonstrably runs beside the null stream is used, and all four are given back, also when the set-up fails."""
    torch = torch_cuda
    binding.lib()
    hip = _hip_runtime()
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    torch.zeros(1, device="cuda")
    raw = []
    for _ in range(4):
        h = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(h), 1) == 0            # hipStreamNonBlocking
        raw.append(h)
    try:
        side = None
        probe = torch.zeros(1, device="cuda")
        for h in raw:
            cand = torch.cuda.ExternalStream(h.value)
            torch.cuda.synchronize()
            with torch.cuda.stream(cand):
                torch.cuda._sleep(50000000)                                    # some 20 ms
            probe.add_(1)                                                      # on the null stream
            torch.cuda.default_stream().synchronize()
            beside = not cand.query()
            cand.synchronize()
            if beside:
                side = cand
                break
        assert side is not None, "no stream runs beside the null stream"
        yield _Gates(torch, side)
    finally:
        torch.cuda.synchronize()
        for h in raw:
            hip.hipStreamDestroy(h)


class Setup:
    pass


@pytest.fixture(scope="module")
def setup(torch_cuda):
    torch = torch_cuda
    s = Setup()
    s.m, s.o = build_pair(cc.KEYWORDS, 1)
    s.plan = s.m.plan(0)
    s.real, s.decoy = np.frombuffer(cc.valid_text(41, N), np.uint8), np.frombuffer(cc.valid_text(42, N), np.uint8)
    rng = np.random.default_rng(43)
    s.off = np.concatenate([[0, 0], np.sort(rng.integers(0, N + 1, size=30)), [N, N]]).astype(np.uint64)
    s.T = s.off.size - 1
    s.d_off = sc.dev(torch, s.off)
    s.rec, s.rec_decoy = s.o.scan(s.real), s.o.scan(s.decoy)
    s.n = min(s.rec.size, s.rec_decoy.size)
    assert 64 <= s.n and max(s.rec.size, s.rec_decoy.size) <= CAP and not np.array_equal(s.rec[:s.n], s.rec_decoy[:s.n])
    # the rulers of both texts, built on the null stream over buffers on the 16-byte grid (as every buffer of a Run is)
    s.rulers = []
    for text in (s.real, s.decoy):
        d = sc.dev(torch, text)
        assert d.data_ptr() % 16 == 0
        s.rulers.append(s.plan.chars_ruler(d).cpu().numpy())
        torch.cuda.synchronize()
    s.plan.status()
    s.pos = np.arange(N + 1, dtype=np.int64)
    s.d_pos = sc.dev(torch, s.pos)
    s.keep = []
    return s


def _records_want(s, text, rec):
    start, length, edge = cc.records_expected(text, rec, s.off, UNIT)
    return [sc.i64(start), sc.i32(length), edge]


def _case(torch, s, name):
    L, h, T, off = binding.lib(), s.plan.h, s.T, s.d_off.data_ptr()
    if name == "acm_gpu_chars_ruler_device":
        rb, tb = L.acm_gpu_chars_ruler_bytes(h, N), L.acm_gpu_chars_ruler_tmp_bytes(h, N)
        tb2 = L.acm_gpu_chars_tmp_bytes(h, N + 1, T)
        tmp2 = torch.zeros(max(tb2, 16), dtype=torch.uint8, device="cuda")
        s.keep.append(tmp2)

        def post(p, st):                                     # every rank of the ruler, through the positions call
            assert L.acm_gpu_chars_positions_device(h, p["text"], N, off, T, UNIT, p["ruler"], s.d_pos.data_ptr(), N + 1, p["out"], tmp2.data_ptr(), tb2,
                                                    st) == 0
        return sc.Case(name, s.plan, lambda p, st: L.acm_gpu_chars_ruler_device(h, p["text"], N, p["ruler"], rb, p["tmp"], tb, st),
                       {"text": (s.real, s.decoy)}, {"ruler": (rb, torch.uint8), "out": (N + 1, torch.int64)}, tb, cut=lambda x: [x["out"]], post=post,
                       want=[sc.i64(cc.positions_expected(s.real, s.pos, s.off, UNIT))])
    if name == "acm_gpu_chars_records_device":
        tb = L.acm_gpu_chars_tmp_bytes(h, CAP, T)
        n = s.n
        gated = {"text": (s.real, s.decoy), "ruler": tuple(s.rulers), "rec": (sc.padded(s.rec[:n], CAP), sc.padded(s.rec_decoy[:n], CAP)),
                 "n": (np.array([n], np.uint64), np.array([n], np.uint64))}
        return sc.Case(name, s.plan,
                       lambda p, st: L.acm_gpu_chars_records_device(h, p["text"], N, 0, off, T, UNIT, p["ruler"], p["rec"], CAP, p["n"], p["start"], p["len"],
                                                                    p["edge"], p["tmp"], tb, st),
                       gated, {"start": (CAP, torch.int64), "len": (CAP, torch.int32), "edge": (CAP, torch.uint8)}, tb,
                       cut=lambda x: [x["start"][:n], x["len"][:n], x["edge"][:n]], want=_records_want(s, s.real, s.rec[:n]))
    if name == "acm_gpu_chars_positions_device":
        tb = L.acm_gpu_chars_tmp_bytes(h, N + 1, T)
        gated = {"text": (s.real, s.decoy), "ruler": tuple(s.rulers)}
        return sc.Case(name, s.plan,
                       lambda p, st: L.acm_gpu_chars_positions_device(h, p["text"], N, off, T, UNIT, p["ruler"], s.d_pos.data_ptr(), N + 1, p["out"], p["tmp"],
                                                                      tb, st),
                       gated, {"out": (N + 1, torch.int64)}, tb, want=[sc.i64(cc.positions_expected(s.real, s.pos, s.off, UNIT))])
    assert name == "acm_gpu_scan_chars_device"
    tb = L.acm_gpu_scan_chars_tmp_bytes(h, CAP, N, T)

    def cut(x):
        k = int(x["count"][0])
        return [sc.rows(x, "rec", k), x["start"][:k], x["len"][:k], x["edge"][:k], x["count"]]
    return sc.Case(name, s.plan,
                   lambda p, st: L.acm_gpu_scan_chars_device(h, p["text"], N, 0, off, T, UNIT, p["rec"], p["start"], p["len"], p["edge"], CAP, p["count"],
                                                             p["tmp"], tb, st),
                   {"text": (s.real, s.decoy)},
                   {"rec": (2 * CAP, torch.int64), "start": (CAP, torch.int64), "len": (CAP, torch.int32), "edge": (CAP, torch.uint8),
                    "count": (1, torch.int64)}, tb, cut=cut, want=[sc.rec_rows(s.rec)] + _records_want(s, s.real, s.rec) + [np.array([s.rec.size])])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_chars_entry_points_on_a_side_stream(torch_cuda, gates, setup, entry):
    bad = sc.exercise(torch_cuda, gates, _case(torch_cuda, setup, entry), control=entry == "acm_gpu_scan_chars_device")
    assert not bad, "\n".join(bad)
