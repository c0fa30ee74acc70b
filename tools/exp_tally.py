"""Experiment driver: what the per-keyword tally (acm_gpu_tally_device, csrc/dev_tally.h) costs beside
the two calls a caller has today, on texts resident on the device:
  (a) acm_gpu_count_device                      -- all matches together, no records;
  (b) acm_gpu_scan_device with records          -- what a caller must run today to get the counts per
                                                   keyword, WITHOUT the download of the records and the
                                                   binning on the host that has to follow;
  (c) acm_gpu_tally_device, windows of 64 MiB   -- the counts per keyword, nothing to download but them,
for config 2's dictionary (1,000 keywords: dense kernel, LDS form of the tally) and config 3's
(100,000 keywords: 4-gram kernel, global form), 1 GiB of synthetic text each, and (c) alone on the
contention case: 64 MiB of 'a' against the keywords a, aa, aaa -- three records per position, every
add on one of three counters.
The three paths alternate inside one timed loop, several rounds; every path is timed with device
events around `steps` calls, the steps chosen so that a round takes about --window seconds.  The
tally's counters are checked against (a)'s count before anything is timed.
Writes the numbers to --out (JSON) and prints them."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import lib, _check

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "tally.json"))
ap.add_argument("--log2", type=int, default=30, help="text size of the two configurations")
ap.add_argument("--window-log2", type=int, default=26, help="tally window")
ap.add_argument("--contention-log2", type=int, default=26)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed round")
ap.add_argument("--only", default="", help="config2 / config3 / contention: that part alone (profiling runs)")
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


def tally_call(plan, text, n, window, capacity):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    counters = torch.zeros(max(plan.tally_keywords, 1), dtype=torch.int64, device="cuda")
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_tally_tmp_bytes(plan.h, window, capacity)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call():
        _check(L.acm_gpu_tally_device(plan.h, text.data_ptr(), n, 0, counters.data_ptr(), counters.numel(), window, capacity, out.data_ptr(),
                                      out.data_ptr() + 8, tmp.data_ptr(), tb, st), "acm_gpu_tally_device")
    return call, counters, out


def run_config(name, K, n):
    kd, ko = acm.synth.keywords(K)
    m = acm.Machine(1)
    m.add_keywords_packed(kd, ko)
    plan = m.plan(0)
    text = acm.synth.device_text(n, kd, ko)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    whole = int(plan.count(text, count=cnt).item())
    rec = torch.empty((whole + 1024, 2), dtype=torch.int64, device="cuda")
    window = min(1 << args.window_log2, n)
    # room for the densest window: measured once with a count per window
    densest = max(int(plan.count(text[b:b + window], count=cnt).item()) for b in range(0, n, window))
    capacity = densest + densest // 8 + 4096
    tally, counters, out = tally_call(plan, text, n, window, capacity)
    tally()
    total, need = (int(x) for x in out.cpu())
    assert total == whole == int(counters.sum().item()) and need <= capacity, (total, whole, need, capacity)
    counters.zero_()
    res, steps = measure({"a_count": lambda: plan.count(text, count=cnt),
                          "b_scan_records": lambda: plan.scan(text, records=rec, count=cnt),
                          "c_tally": tally})
    plan.status()
    a, b, c = (res[k][0] for k in ("a_count", "b_scan_records", "c_tally"))
    case = {"keywords": K, "text_bytes": n, "kernel": int(plan.info.kernel), "tally_form": plan.tally_form, "records": whole,
            "record_bytes_b_would_download": whole * 16, "tally_bytes_c_downloads": K * 8,
            "tally_window_symbols": window, "tally_capacity_records": capacity, "largest_window_records": need, "steps_per_round": steps,
            "a_count_ms": a, "b_scan_records_ms": b, "c_tally_ms": c, "c_minus_b_ms": c - b, "c_over_b": c / b,
            "rounds_ms": {k: v[1] for k, v in res.items()}}
    print(name, json.dumps(case), flush=True)
    return case


def run_contention(n):
    m = acm.Machine(1)
    for kw in (b"a", b"aa", b"aaa"):
        m.add_keyword(kw)
    plan = m.plan(0)
    text = torch.full((n,), ord("a"), dtype=torch.uint8, device="cuda")
    window, cases = 1 << 22, {}
    capacity = 3 * window
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rec = torch.empty((3 * n, 2), dtype=torch.int64, device="cuda")
    for form in ("lds", "global"):
        if form == "global":
            os.environ["ACM_GPU_TALLY"] = "global"
        tally, counters, out = tally_call(plan, text, n, window, capacity)
        tally()
        assert counters.cpu().tolist() == [n, n - 1, n - 2] and int(out[0].item()) == 3 * n - 3
        res, steps = measure({"b_scan_records": lambda: plan.scan(text, records=rec, count=cnt), "c_tally": tally})
        cases[form] = {"tally_form": plan.tally_form, "b_scan_records_ms": res["b_scan_records"][0], "c_tally_ms": res["c_tally"][0],
                       "c_minus_b_ms": res["c_tally"][0] - res["b_scan_records"][0], "steps_per_round": steps,
                       "rounds_ms": {k: v[1] for k, v in res.items()}}
        os.environ.pop("ACM_GPU_TALLY", None)
    plan.status()
    case = {"text_bytes": n, "records": 3 * n - 3, "tally_window_symbols": window, "tally_capacity_records": capacity, "forms": cases}
    print("contention", json.dumps(case), flush=True)
    return case


out = {"what": "tools/exp_tally.py: ms per call, medians of %d rounds of about %.1f s each, the paths alternating, device events; "
               "(a) = acm_gpu_count_device, (b) = acm_gpu_scan_device with records (no download), (c) = acm_gpu_tally_device" % (args.rounds, args.window),
       "device": torch.cuda.get_device_name(0)}
if args.only in ("", "config2"):
    out["config2"] = run_config("config2", 1000, 1 << args.log2)
    torch.cuda.empty_cache()
if args.only in ("", "config3"):
    out["config3_dictionary"] = run_config("config3", 100000, 1 << args.log2)
    torch.cuda.empty_cache()
if args.only in ("", "contention"):
    out["contention_all_a"] = run_contention(1 << args.contention_log2)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
