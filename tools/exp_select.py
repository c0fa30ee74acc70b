"""Experiment driver: what the leftmost-longest selection costs beside the ordered scan it runs behind.
acm_gpu_scan_select_device is acm_gpu_scan_ordered_device (emit_from = 0) plus the passes of
csrc/dev_select.h over the records.  This times, in one process and on one build, on a text resident
on the device,
  (a) acm_gpu_scan_ordered_device of the buffer;
  (b) acm_gpu_scan_select_device of the same buffer into the same record room,
for the 1,000-keyword synthetic dictionary on 64 Mi byte symbols.  (a) and (b) alternate inside one
timed loop, several rounds, every round ending in a device synchronise; ms per call, medians.  The
expectation from the passes is (b) = (a) + about 150 bytes of traffic per record and
the resolve kernel's serial chain.  Prints one JSON line and writes it to --out if given."""
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
ap.add_argument("--out", default=None)
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--keywords", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
n = 1 << args.log2


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


kd, ko = acm.synth.keywords(args.keywords)
m = acm.Machine(1)
m.add_keywords_packed(kd, ko)
plan = m.plan(0)
text = acm.synth.device_text(n, kd, ko)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
cap = int(plan.count(text).item()) + 4096
rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
to = L.acm_gpu_scan_ordered_tmp_bytes(plan.h, cap, n)
ts = L.acm_gpu_scan_select_tmp_bytes(plan.h, cap, n)
tmp = torch.empty(max(to, ts), dtype=torch.uint8, device="cuda")


def ordered():
    _check(L.acm_gpu_scan_ordered_device(plan.h, text.data_ptr(), n, 0, 0, rec.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), to, st),
           "acm_gpu_scan_ordered_device")


def select():
    _check(L.acm_gpu_scan_select_device(plan.h, text.data_ptr(), n, 0, rec.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), ts, st),
           "acm_gpu_scan_select_device")


ordered()
torch.cuda.synchronize()
records_in = int(cnt.item())
for fn in (select, ordered, select):                              # warm-up of both shapes
    fn()
torch.cuda.synchronize()
records_out = int(cnt.item())
assert 0 < records_out <= records_in <= cap
plan.status()
steps = max(5, int(args.window * 1e3 / max(timed(select, 5), 1e-3)))
a, b = [], []
for _ in range(args.rounds):                                      # alternating, so that drift hits both alike
    a.append(timed(ordered, steps))
    b.append(timed(select, steps))
am, bm = float(np.median(a)), float(np.median(b))
case = {"keywords": args.keywords, "text_bytes": n, "kernel": int(plan.info.kernel), "select_form": plan.select_form,
        "records_in": records_in, "records_out": records_out, "steps_per_round": steps, "tmp_bytes_ordered": int(to),
        "tmp_bytes_select": int(ts), "a_scan_ordered_ms": am, "a_rounds_ms": a, "b_scan_select_ms": bm, "b_rounds_ms": b,
        "b_minus_a_ms": bm - am, "b_over_a": bm / am, "b_minus_a_ns_per_record_in": (bm - am) * 1e6 / records_in}
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_select.py: ms per call, medians of %d rounds of about %.1f s each, (a) and (b) alternating" % (
            args.rounds, args.window), "device": torch.cuda.get_device_name(0), "case": case}, f, indent=1)
        f.write("\n")
