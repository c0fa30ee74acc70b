"""Measurement driver: what the map of byte positions to code points and UTF-16 units (include/acm_chars.h,
csrc/dev_chars.h) costs, and which chunk C and tile T its ruler should have, on config 2's workload (bench.py: 1,000
synthetic ASCII keywords, --mib MiB of synthetic text, 1024 by default) and its ordered record set.
  ruler     acm_gpu_chars_ruler_device under every C in 64, 128, 256 (at the default T, 64 Ki) and every T in 4 Ki .. 256 Ki (at
            every C's best neighbour, 128), beside acm_gpu_split_device counting only over the same buffer: the existing
            pass that reads a text once;
  map       acm_gpu_chars_records_device under every C, beside acm_gpu_words_records_device on the same records;
  fused     acm_gpu_scan_chars_device beside acm_gpu_scan_ordered_device alone.
All calls alternate inside one timed loop with device events around `steps` calls, several rounds, the median.  Before
anything is timed the three calls are checked: on this text (ASCII: a position is its byte index) on the device, and on
4 MiB of valid UTF-8 with characters of every width against acm_chars_records on the host, under every C.
Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import lib, _check

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chars.json"))
ap.add_argument("--mib", type=int, default=1024, help="MiB of config 2's text")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
CHUNKS, TILES = (64, 128, 256), (4096, 16384, 65536, 262144)
UNIT = binding.ACM_CHARS_UTF16


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def measure(fns):
    """{name: (median ms, rounds)} of the calls in fns, alternating, after a warm-up of every one"""
    for fn in list(fns.values()) * 2:
        fn()
    torch.cuda.synchronize()
    slowest = max(timed(fn, 3) for fn in fns.values())
    steps = max(3, int(args.window * 1e3 / max(slowest, 1e-3)))
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            rounds[k].append(timed(fn, steps))
    return {k: (float(np.median(v)), v) for k, v in rounds.items()}, steps


def geometry(chunk=None, tile=None):
    for name, v in (("ACM_GPU_CHARS_CHUNK", chunk), ("ACM_GPU_CHARS_TILE", tile)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)


kd, ko = acm.synth.keywords(1000)
m = acm.Machine(1)
m.add_keywords_packed(kd, ko)
plan = m.plan(0)
n = args.mib << 20
text = acm.synth.device_text(n, kd, ko, device="cuda:0")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
whole = int(plan.count(text).item())
cap = whole + 4096
records, count, _ = plan.scan_ordered(text, capacity=cap)
torch.cuda.synchronize()
assert int(count.item()) == whole

# ---- the checks: valid UTF-8 of every width against the host definition, then this text on the device
sys.path.insert(0, os.path.join(ROOT, "tests"))
from chars_cases import KEYWORDS, valid_text                                     # noqa: E402

small = np.frombuffer(valid_text(1, 4 << 20), np.uint8)
ms = acm.Machine(1)
for kw in KEYWORDS:
    ms.add_keyword(kw)
ps = ms.plan(0)
for chunk in CHUNKS:
    geometry(chunk)
    for mis in (0, 5):
        d = torch.zeros(small.size + 16, dtype=torch.uint8, device="cuda")[mis:mis + small.size]
        d.copy_(torch.from_numpy(small.copy()))
        rec, s, ln, e, cnt, _ = ps.scan_chars(d, unit=UNIT, capacity=1 << 22)
        k = int(cnt.item())
        host_rec = np.frombuffer(rec[:k].cpu().numpy().tobytes(), binding.RECORD_DTYPE)
        hs, hl, he = binding.chars_records(small, host_rec, unit=UNIT)
        assert k > 100000 and np.array_equal(s[:k].cpu().numpy().view(np.uint64), hs) and np.array_equal(ln[:k].cpu().numpy().view(np.uint32), hl)
        assert np.array_equal(e[:k].cpu().numpy(), he) and he.any() and not he.all()
    ps.status()
geometry()

start = torch.zeros(cap, dtype=torch.int64, device="cuda")
length = torch.zeros(cap, dtype=torch.int32, device="cuda")
edge = torch.zeros(cap, dtype=torch.uint8, device="cuda")
geometry(64, 4096)                                                               # the largest ruler and scratch of the sweep
rb, rt = L.acm_gpu_chars_ruler_bytes(plan.h, n), L.acm_gpu_chars_ruler_tmp_bytes(plan.h, n)
geometry()
rulers = {c: torch.empty(rb, dtype=torch.uint8, device="cuda") for c in CHUNKS}
sweep = torch.empty(rb, dtype=torch.uint8, device="cuda")
r_tmp = torch.empty(rt, dtype=torch.uint8, device="cuda")
mt = L.acm_gpu_chars_tmp_bytes(plan.h, cap, 0)
m_tmp = torch.empty(max(mt, 16), dtype=torch.uint8, device="cuda")


def ruler(into, chunk=None, tile=None):
    geometry(chunk, tile)
    _check(L.acm_gpu_chars_ruler_device(plan.h, text.data_ptr(), n, into.data_ptr(), rb, r_tmp.data_ptr(), rt, st), "acm_gpu_chars_ruler_device")


def chars_map(chunk):
    _check(L.acm_gpu_chars_records_device(plan.h, text.data_ptr(), n, 0, None, 0, UNIT, rulers[chunk].data_ptr(), records.data_ptr(), cap, count.data_ptr(),
                                          start.data_ptr(), length.data_ptr(), edge.data_ptr(), m_tmp.data_ptr(), mt, st), "acm_gpu_chars_records_device")


for c in CHUNKS:
    ruler(rulers[c], c)
    chars_map(c)
    host = records[:whole].cpu().numpy().view(np.uint64).reshape(-1, 2)
    s0 = host[:, 0] + 1 - (host[:, 1] & 0xFFFFFFFF)
    assert np.array_equal(start[:whole].cpu().numpy().view(np.uint64), s0) and np.array_equal(length[:whole].cpu().numpy().view(np.uint32), (host[:, 1] & 0xFFFFFFFF).astype(np.uint32))
    assert not edge[:whole].any()
plan.status()

# ---- the passes beside them
delim, nd = binding._delims(b"q", 1)
s_bytes = L.acm_gpu_split_tmp_bytes(plan.h, n)
s_tmp = torch.empty(s_bytes, dtype=torch.uint8, device="cuda")
n_texts = torch.zeros(1, dtype=torch.int64, device="cuda")


def split_count():
    _check(L.acm_gpu_split_device(plan.h, text.data_ptr(), n, delim.ctypes.data, nd, binding.ACM_SPLIT_EVERY, None, 0, n_texts.data_ptr(), s_tmp.data_ptr(),
                                  s_bytes, st), "acm_gpu_split_device")


wr, nr = binding._word_ranges(binding.ASCII_WORD, 1)
w_bytes = L.acm_gpu_words_tmp_bytes(plan.h, cap, 0)
w_tmp = torch.empty(w_bytes, dtype=torch.uint8, device="cuda")
w_out = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
w_count = torch.zeros(1, dtype=torch.int64, device="cuda")


def words():
    _check(L.acm_gpu_words_records_device(plan.h, text.data_ptr(), n, 0, None, 0, wr.ctypes.data, nr, binding.ACM_WORDS_BOTH, records.data_ptr(), cap,
                                          count.data_ptr(), w_out.data_ptr(), w_count.data_ptr(), w_tmp.data_ptr(), w_bytes, st), "acm_gpu_words_records_device")


o_bytes = L.acm_gpu_scan_ordered_tmp_bytes(plan.h, cap, n)
geometry(64, 4096)
f_bytes = L.acm_gpu_scan_chars_tmp_bytes(plan.h, cap, n, 0)
geometry()
o_tmp = torch.empty(o_bytes, dtype=torch.uint8, device="cuda")
f_tmp = torch.empty(f_bytes, dtype=torch.uint8, device="cuda")
f_rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
f_count = torch.zeros(1, dtype=torch.int64, device="cuda")


def ordered():
    _check(L.acm_gpu_scan_ordered_device(plan.h, text.data_ptr(), n, 0, 0, f_rec.data_ptr(), cap, f_count.data_ptr(), o_tmp.data_ptr(), o_bytes, st),
           "acm_gpu_scan_ordered_device")


def fused():
    geometry()
    _check(L.acm_gpu_scan_chars_device(plan.h, text.data_ptr(), n, 0, None, 0, UNIT, f_rec.data_ptr(), start.data_ptr(), length.data_ptr(), edge.data_ptr(), cap,
                                       f_count.data_ptr(), f_tmp.data_ptr(), f_bytes, st), "acm_gpu_scan_chars_device")


fns = {"split_count": split_count, "words_records": words, "scan_ordered": ordered, "scan_chars": fused}
for c in CHUNKS:
    fns["ruler_C%d" % c] = lambda c=c: ruler(sweep, c)
    fns["map_C%d" % c] = lambda c=c: chars_map(c)
for t in TILES:
    fns["ruler_T%d" % t] = lambda t=t: ruler(sweep, 128, t)
t, steps = measure(fns)
geometry()
plan.status()
ms_of = {k: v[0] for k, v in t.items()}
out = {"what": "tools/exp_chars.py: ms per call; medians of %d rounds of about %.1f s each, all calls alternating, device events" % (args.rounds, args.window),
       "device": torch.cuda.get_device_name(0), "keywords": 1000, "kernel": int(plan.info.kernel), "text_bytes": n, "records": whole,
       "steps_per_round": steps, "ms": ms_of,
       "ruler_GBps": {k: n / (v * 1e6) for k, v in ms_of.items() if k.startswith("ruler_")}, "split_count_GBps": n / (ms_of["split_count"] * 1e6),
       "map_records_per_s": {k: whole / (v * 1e-3) for k, v in ms_of.items() if k.startswith("map_")},
       "words_records_per_s": whole / (ms_of["words_records"] * 1e-3),
       "ruler_bytes": {str(c): int([geometry(c), L.acm_gpu_chars_ruler_bytes(plan.h, n)][1]) for c in CHUNKS},
       "scan_chars_over_scan_ordered": ms_of["scan_chars"] / ms_of["scan_ordered"], "defaults": {"chunk": 128, "tile": 65536},
       "rounds_ms": {k: v[1] for k, v in t.items()}}
geometry()
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump([out], f, indent=1)
    f.write("\n")
print("wrote", args.out)
