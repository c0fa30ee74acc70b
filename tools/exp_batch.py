"""Experiment driver: what a batch scan costs beside the ordered scan of the same buffer.
acm_gpu_scan_batch_device is acm_gpu_scan_ordered_device of the concatenation plus one pass over
its records (csrc/dev_batch.h); this times, on texts resident on the device,
  (a) Plan.scan_ordered of the concatenation -- the yardstick, the code every scan ran before;
  (b) the batch scan of the same buffer cut into texts of a mean of 64 B, 1 KiB and 64 KiB (one
      cut point in 50 doubled, so that empty texts occur) -- the raw acm_gpu_scan_batch_device call
      with its buffers allocated beforehand, as (a) is timed; what the Python wrapper
      Plan.scan_batch adds on top (its count pass, allocations, the download) is timed apart on
      config 2 (b_python_scan_batch_ms);
  (c) for scale, one Plan.scan_ordered call per text over the first 10,000 texts of the 1 KiB
      case, extrapolated to all of them,
for config 2 (1,000 keywords, 1 GiB) and config 3's dictionary (100,000 keywords) on a text whose
records fit beside it (256 MiB by default: some 107 M records).  (a) and (b) alternate inside one
timed loop, several rounds, every round ending in a device synchronise; ms per step.  The steps of
a round are chosen so that a round takes about --window seconds (a call of config 2 is a third of a
millisecond: ten of them would time the clock).
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "batch_scan.json"))
ap.add_argument("--c2-log2", type=int, default=30)
ap.add_argument("--c3-log2", type=int, default=28)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed round")
ap.add_argument("--per-text", type=int, default=10000)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()


def cuts(n, mean):
    """offsets of n symbols cut at n // mean random points (seeded), on the device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    c = torch.randint(0, n + 1, (n // mean,), generator=g, device="cuda", dtype=torch.int64)
    c = torch.cat([c, c[::50]])                                   # doubled cut points: empty texts
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.sort(c).values, torch.full((1,), n, dtype=torch.int64, device="cuda")])
    return off.contiguous()


def run_config(name, K, n):
    kd, ko = acm.synth.keywords(K)
    m = acm.Machine(1)
    m.add_keywords_packed(kd, ko)
    plan = m.plan(0)
    text = acm.synth.device_text(n, kd, ko)
    whole = int(plan.count(text).item())
    cap = whole + 1024
    rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    tid = torch.empty(cap, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    otmp = None
    res = {"keywords": K, "text_bytes": n, "kernel": int(plan.info.kernel), "records_in_the_concatenation": whole, "cases": []}

    def ordered():
        nonlocal otmp
        _, _, otmp = plan.scan_ordered(text, records=rec, count=cnt, tmp=otmp)

    for mean in (64, 1024, 65536):
        off = cuts(n, mean)
        n_texts = off.numel() - 1
        first = torch.empty(n_texts + 1, dtype=torch.int64, device="cuda")
        tb = L.acm_gpu_scan_batch_tmp_bytes(plan.h, cap, n, n_texts)
        btmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

        def batch():
            _check(L.acm_gpu_scan_batch_device(plan.h, text.data_ptr(), n, off.data_ptr(), n_texts, rec.data_ptr(), tid.data_ptr(), first.data_ptr(),
                                               cap, cnt.data_ptr(), btmp.data_ptr(), tb, st), "acm_gpu_scan_batch_device")

        def timed(fn, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        for fn in (ordered, batch, ordered, batch):              # warm-up of both shapes
            fn()
        torch.cuda.synchronize()
        kept = int(cnt.item())
        assert int(first[-1].item()) == kept and kept <= whole
        plan.status()
        steps = max(10, int(args.window * 1e3 / max(timed(batch, 10), 1e-3)))
        a, b = [], []
        for _ in range(args.rounds):                             # alternating, so that drift hits both alike
            a.append(timed(ordered, steps))
            b.append(timed(batch, steps))
        am, bm = float(np.median(a)), float(np.median(b))
        case = {"mean_text_bytes": mean, "texts": n_texts, "empty_texts": int((off[1:] == off[:-1]).sum().item()),
                "batch_records": kept, "dropped": whole - kept, "steps_per_round": steps,
                "a_scan_ordered_ms": am, "a_rounds_ms": a, "b_scan_batch_ms": bm, "b_rounds_ms": b,
                "b_minus_a_ms": bm - am, "b_minus_a_ms_per_million_records": (bm - am) / (whole / 1e6), "b_over_a": bm / am}
        if name == "config2":
            t0 = time.perf_counter()
            for _ in range(5):
                plan.scan_batch(text, off)
            case["b_python_scan_batch_ms"] = (time.perf_counter() - t0) / 5 * 1e3
        if mean == 1024:
            # (c) one ordered scan per text, buffers reused, one synchronise at the end
            k = min(args.per_text, n_texts)
            host_off = off[:k + 1].cpu().numpy()
            small = torch.empty((4096, 2), dtype=torch.int64, device="cuda")
            stmp = None
            for t in range(100):
                _, _, stmp = plan.scan_ordered(text[int(host_off[t]):int(host_off[t + 1])], records=small, count=cnt, tmp=stmp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(k):
                _, _, stmp = plan.scan_ordered(text[int(host_off[t]):int(host_off[t + 1])], records=small, count=cnt, tmp=stmp)
            torch.cuda.synchronize()
            per = (time.perf_counter() - t0) / k * 1e3
            case.update({"c_texts_timed": k, "c_ms_per_text": per, "c_extrapolated_ms": per * n_texts, "c_over_b": per * n_texts / bm})
        print(name, json.dumps(case), flush=True)
        res["cases"].append(case)
        del btmp, first, off
    return res


out = {"what": "tools/exp_batch.py: ms per step, medians of %d rounds of about %.1f s each, (a) and (b) alternating; "
               "(a) = Plan.scan_ordered, (b) = acm_gpu_scan_batch_device with buffers allocated beforehand, "
               "b_python_scan_batch_ms = Plan.scan_batch (count pass, allocations, download), (c) = one Plan.scan_ordered per text" % (args.rounds, args.window),
       "device": torch.cuda.get_device_name(0),
       "config2": run_config("config2", 1000, 1 << args.c2_log2)}
torch.cuda.empty_cache()
out["config3_dictionary"] = run_config("config3", 100000, 1 << args.c3_log2)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
