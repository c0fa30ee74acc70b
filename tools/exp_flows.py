"""Experiment driver: what a flow scan costs beside the batch scan of the same buffer.
acm_gpu_scan_flows_device is acm_gpu_scan_batch_device over a second buffer that holds every text
behind its flow's carry, plus the passes that make that buffer and keep the carries
(csrc/dev_flows.h).  This times, in one process and on one build, on a text resident on the device,
  (a) acm_gpu_scan_batch_device of the buffer -- the call as it was before flows existed;
  (b) acm_gpu_scan_flows_device of the same buffer and offsets, every text a flow of its own under
      a random permutation of the ids, the flows warm (every carry full: the steady state),
for the 1,000-keyword synthetic dictionary on 64 Mi byte symbols cut into texts of a mean of 64 and
of 1,024 symbols.  (a) and (b) alternate inside one timed loop, several rounds, every round ending in
a device synchronise; ms per call, medians.  The expectation from the passes is (b) = (a) + one read
and one write of the text.  Prints one JSON line per case and writes all of them to --out if given."""
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


def cuts(n, mean):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    c = torch.randint(0, n + 1, (n // mean,), generator=g, device="cuda", dtype=torch.int64)
    c = torch.cat([c, c[::50]])                                   # doubled cut points: empty texts
    return torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.sort(c).values,
                      torch.full((1,), n, dtype=torch.int64, device="cuda")]).contiguous()


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
cases = []
for mean in (64, 1024):
    off = cuts(n, mean)
    n_texts = off.numel() - 1
    flows = plan.flows(n_texts)
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    ids = torch.randperm(n_texts, generator=g, device="cuda").to(torch.int32).contiguous()
    # room for the matches of the buffer with the carries in front: the ordered count and half as much again
    cap = int(plan.count(text).item()) * 3 // 2 + 4096
    rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    tid = torch.empty(cap, dtype=torch.int32, device="cuda")
    first = torch.empty(n_texts + 1, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_scan_batch_tmp_bytes(plan.h, cap, n, n_texts)
    tf = L.acm_gpu_scan_flows_tmp_bytes(plan.h, flows.h, cap, n, n_texts)
    tmp = torch.empty(max(tb, tf), dtype=torch.uint8, device="cuda")

    def batch():
        _check(L.acm_gpu_scan_batch_device(plan.h, text.data_ptr(), n, off.data_ptr(), n_texts, rec.data_ptr(), tid.data_ptr(), first.data_ptr(),
                                           cap, cnt.data_ptr(), tmp.data_ptr(), tb, st), "acm_gpu_scan_batch_device")

    def flow():
        _check(L.acm_gpu_scan_flows_device(plan.h, flows.h, text.data_ptr(), n, off.data_ptr(), ids.data_ptr(), n_texts, rec.data_ptr(),
                                           tid.data_ptr(), first.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), tf, st), "acm_gpu_scan_flows_device")

    batch()
    torch.cuda.synchronize()
    batch_records = int(cnt.item())
    for fn in (flow, batch, flow, batch, flow):                   # warm-up of both shapes; the carries fill
        fn()
    torch.cuda.synchronize()
    flow_records = int(cnt.item())
    assert batch_records <= flow_records <= cap and int(first[-1].item()) == flow_records
    plan.status()
    steps = max(5, int(args.window * 1e3 / max(timed(flow, 5), 1e-3)))
    a, b = [], []
    for _ in range(args.rounds):                                  # alternating, so that drift hits both alike
        a.append(timed(batch, steps))
        b.append(timed(flow, steps))
    am, bm = float(np.median(a)), float(np.median(b))
    case = {"keywords": args.keywords, "text_bytes": n, "mean_text_symbols": mean, "texts": n_texts, "kernel": int(plan.info.kernel),
            "batch_records": batch_records, "flow_records": flow_records, "steps_per_round": steps, "tmp_bytes_batch": int(tb),
            "tmp_bytes_flows": int(tf), "a_scan_batch_ms": am, "a_rounds_ms": a, "b_scan_flows_ms": bm, "b_rounds_ms": b,
            "b_minus_a_ms": bm - am, "b_over_a": bm / am,
            "b_minus_a_GBps_of_one_read_and_one_write_of_the_text": 2 * n / ((bm - am) * 1e-3) / 1e9}
    print(json.dumps(case), flush=True)
    cases.append(case)
    flows.close()
    del rec, tid, first, tmp, off, ids
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_flows.py: ms per call, medians of %d rounds of about %.1f s each, (a) and (b) alternating" % (
            args.rounds, args.window), "device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
        f.write("\n")
