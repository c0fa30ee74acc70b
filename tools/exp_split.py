"""Experiment driver: what cutting a buffer into texts on the device (acm_gpu_split_device,
csrc/dev_split.h) costs beside the route it replaces and beside the scan it feeds, on one buffer of
synthetic text (config 2's: 1,000 keywords, a-z) with a newline written at pseudo-random gaps of mean 64:
  (1) acm_gpu_split_device, ACM_SPLIT_EVERY, one delimiter  -- count pass, prefix sum, write pass; also
                                                               the count run alone, RUNS, and 16 delimiters;
  (2) the host route: the text in host memory, np.flatnonzero (text == 10) + 1, the offsets uploaded
                                                            -- a host clock around work that ends in a
                                                               device synchronise; the download of the
                                                               text that a device-resident caller pays
                                                               first is timed beside it;
  (3) acm_gpu_count_device of the same buffer on the dense plan -- the scan the split feeds;
and a plain device-to-device copy and a read (sum) of the same buffer, tools/exp_membw.py's figures at
this size.  (1) and (3) and the copy alternate inside one timed loop, several rounds, device events
around `steps` calls.  (1)'s offsets are checked against numpy's before anything is timed.
Writes the numbers to --out (JSON) and prints them."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import lib, _check

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "split.json"))
ap.add_argument("--log2", type=int, default=30, help="text size")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed round")
ap.add_argument("--host-reps", type=int, default=3)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()


def timed(fn, steps):
    """ms per call: device events around `steps` calls"""
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


n = 1 << args.log2
K = 1000
kd, ko = acm.synth.keywords(K)
m = acm.Machine(1)
m.add_keywords_packed(kd, ko)
plan = m.plan(0)
text = acm.synth.device_text(n, kd, ko)
rng = np.random.default_rng(5)
at = np.cumsum(rng.integers(1, 128, size=n // 64 + n // 640))              # gaps of 1 .. 127: mean 64
at = at[at < n]
text[torch.from_numpy(at).cuda()] = 10
host = text.cpu().numpy()
want = np.concatenate([[0], np.flatnonzero(host == 10) + 1, [n] if host[-1] != 10 else []]).astype(np.int64)
n_texts = want.size - 1
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
nl = np.frombuffer(b"\n", np.uint8)
sixteen = np.frombuffer(b"\n\t ,;.:!?()[]{}-", np.uint8)
tb = L.acm_gpu_split_tmp_bytes(plan.h, n)
tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
off = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")


def split(delims=nl, flags=0, offsets=True):
    _check(L.acm_gpu_split_device(plan.h, text.data_ptr(), n, delims.ctypes.data, delims.size, flags, off.data_ptr() if offsets else None, n_texts,
                                  cnt.data_ptr(), tmp.data_ptr(), tb, st), "acm_gpu_split_device")


split()
assert int(cnt.item()) == n_texts and np.array_equal(off.cpu().numpy(), want)
split(offsets=False)
assert int(cnt.item()) == n_texts
split(delims=sixteen)                                                      # (the text is a-z and newlines: the same cuts)
assert int(cnt.item()) == n_texts and np.array_equal(off.cpu().numpy(), want)

count = torch.zeros(1, dtype=torch.int64, device="cuda")
other = torch.empty_like(text)
r, steps = measure({"split": split, "split_count_only": lambda: split(offsets=False), "split_runs": lambda: split(flags=1),
                    "split_16_delims": lambda: split(delims=sixteen), "count_scan": lambda: plan.count(text, count=count),
                    "copy": lambda: other.copy_(text), "read": lambda: text.view(torch.int64).sum()})
del other


def host_route(download):
    """seconds: the offsets made on the host and uploaded, the text taken off the device first or not"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = text.cpu().numpy() if download else host
    o = np.flatnonzero(h == 10) + 1
    d = torch.from_numpy(o).cuda()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, d


host_ms = [host_route(False)[0] * 1e3 for _ in range(args.host_reps)]
host_dl_ms = [host_route(True)[0] * 1e3 for _ in range(args.host_reps)]
ms = {k: v[0] for k, v in r.items()}
gb = n / 1e9
out = {"what": "tools/exp_split.py: ms per call, medians of %d rounds of about %.1f s each, the device paths alternating, device events; the host "
               "route by a host clock around work that ends in a synchronise, median of %d" % (args.rounds, args.window, args.host_reps),
       "device": torch.cuda.get_device_name(0), "text_bytes": n, "texts": n_texts, "keywords": K, "kernel": int(plan.info.kernel),
       "tile_bytes": int(os.environ.get("ACM_GPU_SPLIT_TILE", 16384)), "steps_per_round": steps,
       "1_split_ms": ms["split"], "1_split_text_GBps": gb / ms["split"] * 1e3,
       "1_split_traffic_GBps": (2 * n + 8 * n_texts) / 1e9 / ms["split"] * 1e3,
       "1_split_count_only_ms": ms["split_count_only"], "1_split_runs_ms": ms["split_runs"], "1_split_16_delims_ms": ms["split_16_delims"],
       "2_host_route_ms": float(np.median(host_ms)), "2_host_route_with_download_ms": float(np.median(host_dl_ms)),
       "3_count_scan_ms": ms["count_scan"], "3_count_scan_text_GBps": gb / ms["count_scan"] * 1e3,
       "copy_ms": ms["copy"], "copy_traffic_GBps": 2 * gb / ms["copy"] * 1e3, "read_ms": ms["read"], "read_GBps": gb / ms["read"] * 1e3,
       "split_over_read": ms["split"] / ms["read"], "split_over_count_scan": ms["split"] / ms["count_scan"],
       "host_route_over_split": float(np.median(host_ms)) / ms["split"],
       "rounds_ms": {k: v[1] for k, v in r.items()}, "host_rounds_ms": host_ms, "host_with_download_rounds_ms": host_dl_ms}
print(json.dumps(out), flush=True)
plan.status()
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
