"""Experiment driver: what the minimum-cost tiling costs beside the greedy selection.
acm_gpu_scan_segment_device and acm_gpu_scan_select_device are both the ordered scan plus passes over
its records (csrc/dev_segment.h, csrc/dev_select.h).  This times, in one process and on one build, on a
text resident on the device,
  (a) acm_gpu_scan_ordered_device of the buffer;
  (b) acm_gpu_scan_select_device of the same buffer into the same record room;
  (c) acm_gpu_scan_segment_device of it, costs 1 + (id % 5), gap_cost 8,
on two workloads of 64 Mi byte symbols: the 1,000-keyword synthetic dictionary on its synthetic text
(bench.py's config 2) and the novel's own words over the novel repeated.  The three alternate inside one
timed loop, several rounds, every round ending in a device synchronise; ms per call, medians.  The
record and group counts and the longest group come from the records of (a) on the host.  Prints one
JSON line per workload and writes them to --out if given.  `--steps N` fixes the calls per round (a
short run under a kernel trace gives the split between the passes)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import lib, _check, RECORD_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed round")
ap.add_argument("--only", default=None, choices=["synthetic", "novel"])
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
n = 1 << args.log2
GAP = 8


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def groups_of(rec):
    """(number of groups, records of the longest) of records in canonical order: a group begins where the
    least start from the record on exceeds the end in front"""
    end = rec["end_pos"].astype(np.int64)
    start = end + 1 - rec["length"].astype(np.int64)
    low = np.minimum.accumulate(start[::-1])[::-1]
    begins = np.flatnonzero(np.concatenate([[True], low[1:] > end[:-1]]))
    sizes = np.diff(np.concatenate([begins, [rec.size]]))
    return int(begins.size), int(sizes.max())


def workload(name):
    if name == "synthetic":
        kd, ko = acm.synth.keywords(1000)
        m = acm.Machine(1)
        m.add_keywords_packed(kd, ko)
        return m, acm.synth.device_text(n, kd, ko)
    import re
    with open(os.path.join(ROOT, "tests", "golden", "mrs_dalloway.txt"), "rb") as f:
        novel = f.read()
    words = re.findall(rb"[A-Za-z]{3,}", novel)
    seen = {}
    for w in words:
        seen[w] = seen.get(w, 0) + 1
    m = acm.Machine(1)
    for w in sorted(seen, key=lambda w: (-seen[w], w))[:400]:     # its 400 most frequent words of 3 letters or more
        m.add_keyword(w)
    text = np.resize(np.frombuffer(novel, np.uint8), n)
    return m, torch.from_numpy(text.copy()).cuda()


def measure(name):
    m, text = workload(name)
    plan = m.plan(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    sums = torch.zeros(2, dtype=torch.int64, device="cuda")
    cap = int(plan.count(text).item()) + 4096
    rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    cost = torch.from_numpy((1 + np.arange(m.nb_keywords) % 5).astype(np.int32)).cuda()
    to = L.acm_gpu_scan_ordered_tmp_bytes(plan.h, cap, n)
    ts = L.acm_gpu_scan_select_tmp_bytes(plan.h, cap, n)
    tg = L.acm_gpu_scan_segment_tmp_bytes(plan.h, cap, n, 0)
    tmp = torch.empty(max(to, ts, tg), dtype=torch.uint8, device="cuda")

    def ordered():
        _check(L.acm_gpu_scan_ordered_device(plan.h, text.data_ptr(), n, 0, 0, rec.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), to, st),
               "acm_gpu_scan_ordered_device")

    def select():
        _check(L.acm_gpu_scan_select_device(plan.h, text.data_ptr(), n, 0, rec.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), ts, st),
               "acm_gpu_scan_select_device")

    def segment():
        _check(L.acm_gpu_scan_segment_device(plan.h, text.data_ptr(), n, 0, None, 0, cost.data_ptr(), cost.numel(), GAP, rec.data_ptr(), cap,
                                             cnt.data_ptr(), sums.data_ptr(), tmp.data_ptr(), tg, st), "acm_gpu_scan_segment_device")

    ordered()
    torch.cuda.synchronize()
    records_in = int(cnt.item())
    n_groups, longest = groups_of(np.frombuffer(rec[:records_in].cpu().numpy().tobytes(), dtype=RECORD_DTYPE))
    counts = {}
    for fn in (select, segment, ordered, select, segment):        # warm-up of every shape
        fn()
        torch.cuda.synchronize()
        counts[fn.__name__] = int(cnt.item())
    plan.status()
    steps = args.steps or max(3, int(args.window * 1e3 / max(timed(segment, 3), 1e-3)))
    a, b, c = [], [], []
    for _ in range(args.rounds):                                  # alternating, so that drift hits all alike
        a.append(timed(ordered, steps))
        b.append(timed(select, steps))
        c.append(timed(segment, steps))
    am, bm, cm = float(np.median(a)), float(np.median(b)), float(np.median(c))
    case = {"workload": name, "keywords": int(m.nb_keywords), "text_bytes": n, "kernel": int(plan.info.kernel), "records_in": records_in,
            "groups": n_groups, "longest_group_records": longest, "selected": counts["select"], "segmented": counts["segment"],
            "segment_sums": [int(x) for x in sums.tolist()], "steps_per_round": steps, "tmp_bytes_select": int(ts), "tmp_bytes_segment": int(tg),
            "a_scan_ordered_ms": am, "b_scan_select_ms": bm, "c_scan_segment_ms": cm, "a_rounds_ms": a, "b_rounds_ms": b, "c_rounds_ms": c,
            "c_over_b": cm / bm, "passes_select_ms": bm - am, "passes_segment_ms": cm - am,
            "passes_segment_over_select": (cm - am) / (bm - am) if bm > am else None}
    print(json.dumps(case), flush=True)
    plan.close()
    return case


cases = [measure(w) for w in (["synthetic", "novel"] if args.only is None else [args.only])]
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_segment.py: ms per call, medians of %d rounds, (a), (b) and (c) alternating" % args.rounds,
                   "device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
        f.write("\n")
