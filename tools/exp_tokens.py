"""Experiment driver: what tokenising costs beside the selection it runs behind, and beside a plain
copy.  acm_gpu_scan_tokens_device is acm_gpu_scan_select_device (for a batch: the batch scan and the
selection of its records) plus the passes of csrc/dev_tokens.h.  This times, in one process and on one
build, on a text resident on the device (the 1,000-keyword synthetic dictionary on 1 Gi byte symbols,
the workload of tools/exp_replace.py),
  (a) acm_gpu_scan_select_device of the buffer;
  (b) acm_gpu_scan_tokens_device of the same buffer as one text in RUN mode;
  (c) the same in SYMBOL mode (a token per uncovered symbol: ids, starts and lengths are all written);
  (d) a plain device-to-device copy of the buffer on the same stream;
  (e) the batch scan and the selection of the same buffer cut into lines of about 64 symbols;
  (f) acm_gpu_scan_tokens_device of those lines in RUN mode, tok_first included.
The calls alternate inside one timed loop, several rounds, every round ending in a device
synchronise; ms per call, medians.  The token passes' cost is (b) - (a), (c) - (a) and (f) - (e), as
multiples of the copy and of the scan-plus-select in front of them.  Prints one JSON line and writes
it to --out (profiles/tokens.json unless another is given)."""
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
from aho_corasick_1975_amd.binding import lib, _check, TOKENS_GAP_RUN, TOKENS_GAP_SYMBOL

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tokens.json"))
ap.add_argument("--log2", type=int, default=30)
ap.add_argument("--keywords", type=int, default=1000)
ap.add_argument("--line", type=int, default=64, help="mean symbols per line")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
GAP_BASE = 1 << 20


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
n = 1 << args.log2
text = acm.synth.device_text(n, kd, ko)
plan = m.plan(0)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
res = torch.zeros(2, dtype=torch.int64, device="cuda")
cap = int(plan.count(text).item()) + 4096
assert cap < 1 << 31, "more matches than a selection takes"
rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
# lines: a cut every line / 2 .. 3 line / 2 symbols, made on the device from a seed
gen = torch.Generator(device="cuda").manual_seed(64)
steps_ = torch.randint(args.line // 2, args.line * 3 // 2 + 1, (n // (args.line // 2) + 2,), dtype=torch.int64, device="cuda", generator=gen)
cuts = torch.cumsum(steps_, 0)
cuts = cuts[cuts < n]
offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), cuts, torch.full((1,), n, dtype=torch.int64, device="cuda")]).contiguous()
n_texts = offsets.numel() - 1
del steps_, cuts
ts = L.acm_gpu_scan_select_tmp_bytes(plan.h, cap, n)
tb = L.acm_gpu_scan_batch_tmp_bytes(plan.h, cap, n, n_texts)
tt = L.acm_gpu_scan_tokens_tmp_bytes(plan.h, cap, n, n_texts)
tmp = torch.empty(max(ts, tb, tt), dtype=torch.uint8, device="cuda")
first = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")


def select():
    _check(L.acm_gpu_scan_select_device(plan.h, text.data_ptr(), n, 0, rec.data_ptr(), cap, res.data_ptr(), tmp.data_ptr(), ts, st),
           "acm_gpu_scan_select_device")


def batch_select():
    _check(L.acm_gpu_scan_batch_device(plan.h, text.data_ptr(), n, offsets.data_ptr(), n_texts, rec.data_ptr(), None, None, cap, res.data_ptr(),
                                       tmp.data_ptr(), tmp.numel(), st), "acm_gpu_scan_batch_device")
    _check(L.acm_gpu_select_records_device(plan.h, rec.data_ptr(), cap, res.data_ptr(), 0, n, rec.data_ptr(), res.data_ptr(), tmp.data_ptr(),
                                           tmp.numel(), st), "acm_gpu_select_records_device")


def tokens(mode, off, ids, start, length, room):
    _check(L.acm_gpu_scan_tokens_device(plan.h, text.data_ptr(), n, 0, off.data_ptr() if off is not None else None, n_texts if off is not None else 0,
                                        rec.data_ptr(), cap, res.data_ptr(), None, 0, GAP_BASE, mode, ids.data_ptr() if ids is not None else None,
                                        start.data_ptr() if start is not None else None, length.data_ptr() if length is not None else None, room,
                                        res.data_ptr() + 8, first.data_ptr() if off is not None else None, tmp.data_ptr(), tmp.numel(), st),
           "acm_gpu_scan_tokens_device")


def count_tokens(mode, off):
    tokens(mode, off, None, None, None, 0)
    torch.cuda.synchronize()
    return int(res[1].item())


# the two-call pattern: count, then fill
need = {"run": count_tokens(TOKENS_GAP_RUN, None), "symbol": count_tokens(TOKENS_GAP_SYMBOL, None), "lines": count_tokens(TOKENS_GAP_RUN, offsets)}
selected = int(res[0].item())
room = max(need.values())
ids = torch.empty(room, dtype=torch.int32, device="cuda")
start = torch.empty(room, dtype=torch.int64, device="cuda")
length = torch.empty(room, dtype=torch.int32, device="cuda")
copy_to = torch.empty(n, dtype=torch.uint8, device="cuda")
calls = {
    "a_scan_select": select,
    "b_tokens_run": lambda: tokens(TOKENS_GAP_RUN, None, ids, start, length, room),
    "c_tokens_symbol": lambda: tokens(TOKENS_GAP_SYMBOL, None, ids, start, length, room),
    "d_copy": lambda: copy_to.copy_(text[:n]),
    "e_batch_select_lines": batch_select,
    "f_tokens_run_lines": lambda: tokens(TOKENS_GAP_RUN, offsets, ids, start, length, room),
}
for fn in list(calls.values()) * 2:                                 # warm-up of every shape
    fn()
torch.cuda.synchronize()
plan.status()
# the streams agree with their own invariants before anything is timed
tokens(TOKENS_GAP_RUN, offsets, ids, start, length, room)
torch.cuda.synchronize()
assert int(res[1].item()) == need["lines"] and int(length[:need["lines"]].sum(dtype=torch.int64).item()) == n
assert int(first[0].item()) == 0 and int(first[-1].item()) == need["lines"]
ms = {}
for name, fn in calls.items():
    steps = max(3, int(args.window * 1e3 / max(timed(fn, 3), 1e-3)))
    ms[name] = {"steps_per_round": steps, "rounds_ms": []}
for _ in range(args.rounds):                                        # alternating, so that drift hits all alike
    for name, fn in calls.items():
        ms[name]["rounds_ms"].append(timed(fn, ms[name]["steps_per_round"]))
med = {name: float(np.median(v["rounds_ms"])) for name, v in ms.items()}
copy = med["d_copy"]
passes = {"run": med["b_tokens_run"] - med["a_scan_select"], "symbol": med["c_tokens_symbol"] - med["a_scan_select"],
          "run_lines": med["f_tokens_run_lines"] - med["e_batch_select_lines"]}
case = {"case": "config 2 dictionary", "keywords": args.keywords, "text_bytes": n, "kernel": int(plan.info.kernel), "matches": cap - 4096,
        "selected": selected, "n_texts_lines": n_texts, "tokens": need, "tile_symbols": int(os.environ.get("ACM_GPU_TOKENS_TILE", 8192)),
        "tmp_bytes": {"scan_select": int(ts), "scan_batch": int(tb), "scan_tokens": int(tt)}, "median_ms": med, "calls": ms,
        "token_passes_ms": passes, "token_passes_over_copy": {k: v / copy for k, v in passes.items()},
        "token_passes_over_what_they_follow": {"run": passes["run"] / med["a_scan_select"], "symbol": passes["symbol"] / med["a_scan_select"],
                                               "run_lines": passes["run_lines"] / med["e_batch_select_lines"]},
        "copy_GBps_read_plus_write": 2 * n / copy / 1e6}
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_tokens.py: ms per call, medians of %d rounds of about %.1f s each, the six calls alternating" % (
            args.rounds, args.window), "device": torch.cuda.get_device_name(0), "cases": [case]}, f, indent=1)
        f.write("\n")
