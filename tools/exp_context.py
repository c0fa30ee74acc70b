"""Experiment driver: what the context passes cost beside the ordered scan they run behind, and what
their gather moves beside grep's.  acm_gpu_scan_context_device is acm_gpu_scan_ordered_device
(emit_from = 0) plus the passes of csrc/dev_context.h over the records.  This times, in one process
and on one build, on config 2's workload (the 1,000-keyword synthetic dictionary, 1 GiB of a-z text
resident on the device), for windows of (8, 8) and (40, 40) symbols and of (1, 1) texts, all MERGE,
  (a) acm_gpu_scan_ordered_device of the buffer (this change does not touch it);
  (b) acm_gpu_context_records_device alone on the records (a) left, count read on the device, with
      the gather and (b0) without an output buffer: the difference is the gather;
  (c) acm_gpu_scan_context_device of the same buffer: the fused call;
  (g) acm_gpu_grep_device over the same offsets with its gather and (g0) without: the yardstick for
      the copy.  Under TEXTS (0, 0) | MERGE the context output IS grep's gathered output (the texts
      with a match, in order), which is checked byte for byte, and (b) - (b0) is timed for that window
      too: the same bytes moved by both gathers.
The text holds letters only, so its "lines" are texts of --line symbols cut at fixed offsets.
(a) .. (g0) alternate inside one timed loop, several rounds, every round ending in a device
synchronise; ms per call, medians.  Before anything is timed the (8, 8) snippets of the first 64 MiB
are checked against numpy's evaluation of the definition (a cover array).  Prints one JSON line and
writes it to --out if given."""
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
from aho_corasick_1975_amd.binding import lib, _check, RECORD_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--log2", type=int, default=30)
ap.add_argument("--keywords", type=int, default=1000)
ap.add_argument("--line", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
n = 1 << args.log2
SYMBOLS, TEXTS, MERGE = 0, 1, 2


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
offsets = torch.arange(0, n + 1, args.line, dtype=torch.int64, device="cuda")
n_texts = offsets.numel() - 1
cap = int(plan.count(text).item()) + 4096
rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
res = torch.zeros(2, dtype=torch.int64, device="cuda")                  # out_symbols, n_snippets
snip_lo, out_off, rec_at = (torch.zeros(cap + 1, dtype=torch.int64, device="cuda") for _ in range(3))
snip_text, rec_snip = (torch.zeros(cap, dtype=torch.int32, device="cuda") for _ in range(2))
to = L.acm_gpu_scan_ordered_tmp_bytes(plan.h, cap, n)
tc = L.acm_gpu_context_tmp_bytes(plan.h, cap, n_texts)
tf = L.acm_gpu_scan_context_tmp_bytes(plan.h, cap, n, n_texts)
tmp = torch.empty(max(to, tc, tf), dtype=torch.uint8, device="cuda")
out_cap = 3 * args.line * cap                                          # every window of (1, 1) texts on its own
out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
# grep's arrays
g_window, g_cap = 1 << 24, 1 << 20
hits = torch.zeros(n_texts, dtype=torch.int64, device="cuda")
kept = torch.zeros(n_texts, dtype=torch.int32, device="cuda")
g_off = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
g_res = torch.zeros(4, dtype=torch.int64, device="cuda")                # n_kept, total, need, out_symbols
g_out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
tg = L.acm_gpu_grep_tmp_bytes(plan.h, g_window, g_cap, n, n_texts)
g_tmp = torch.empty(tg, dtype=torch.uint8, device="cuda")


def ordered(text=text, n=n):
    _check(L.acm_gpu_scan_ordered_device(plan.h, text.data_ptr(), n, 0, 0, rec.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), to, st),
           "acm_gpu_scan_ordered_device")


def context(before, after, flags, gather=True, text=text, n=n, off=offsets):
    def fn():
        _check(L.acm_gpu_context_records_device(plan.h, text.data_ptr(), n, 0, off.data_ptr() if off is not None else None,
                                                off.numel() - 1 if off is not None else 0, rec.data_ptr(), cap, cnt.data_ptr(), before, after, flags,
                                                out.data_ptr() if gather else None, out_cap if gather else 0, res.data_ptr(), res.data_ptr() + 8,
                                                snip_lo.data_ptr(), out_off.data_ptr(), snip_text.data_ptr(), rec_snip.data_ptr(), rec_at.data_ptr(),
                                                tmp.data_ptr(), tc, st), "acm_gpu_context_records_device")
    return fn


def fused(before, after, flags):
    def fn():
        _check(L.acm_gpu_scan_context_device(plan.h, text.data_ptr(), n, 0, offsets.data_ptr(), n_texts, rec.data_ptr(), cap, cnt.data_ptr(), before,
                                             after, flags, out.data_ptr(), out_cap, res.data_ptr(), res.data_ptr() + 8, snip_lo.data_ptr(),
                                             out_off.data_ptr(), snip_text.data_ptr(), rec_snip.data_ptr(), rec_at.data_ptr(), tmp.data_ptr(), tf, st),
               "acm_gpu_scan_context_device")
    return fn


def grep(gather):
    def fn():
        _check(L.acm_gpu_grep_device(plan.h, text.data_ptr(), n, offsets.data_ptr(), n_texts, 0, g_window, g_cap, hits.data_ptr(), kept.data_ptr(),
                                     g_res.data_ptr(), g_res.data_ptr() + 8, g_res.data_ptr() + 16, g_out.data_ptr() if gather else None,
                                     out_cap if gather else 0, g_off.data_ptr(), g_res.data_ptr() + 24 if gather else None, g_tmp.data_ptr(), tg, st),
               "acm_gpu_grep_device")
    return fn


# the definition on the first 64 MiB, (8, 8) | SYMBOLS | MERGE over one text, with numpy
n_small = min(n, 1 << 26)
ordered(text[:n_small], n_small)
context(8, 8, MERGE, text=text[:n_small], n=n_small, off=None)()
torch.cuda.synchronize()
k = int(cnt.item())
r = np.frombuffer(rec[:k].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
end = r["end_pos"].astype(np.int64)
lo, hi = np.maximum(end + 1 - r["length"] - 8, 0), np.minimum(end + 1 + 8, n_small)
d = np.zeros(n_small + 1, np.int32)
np.add.at(d, lo, 1)
np.add.at(d, hi, -1)
cover = np.concatenate([[False], np.cumsum(d)[:n_small] > 0, [False]])
begins, ends = np.flatnonzero(cover[1:-1] & ~cover[:-2]), np.flatnonzero(cover[1:-1] & ~cover[2:]) + 1
sym, ns = (int(x) for x in res.cpu())
assert ns == begins.size and sym == int((ends - begins).sum()) and 1 < ns < k, (ns, begins.size, sym, k)
assert np.array_equal(snip_lo[:ns].cpu().numpy(), begins)
host = text[:n_small].cpu().numpy()
assert np.array_equal(out[:sym].cpu().numpy(), host[np.flatnonzero(cover[1:-1])])
del d, cover, host
# TEXTS (0, 0) | MERGE is grep's gather
ordered()
context(0, 0, TEXTS | MERGE)()
grep(True)()
torch.cuda.synchronize()
records = int(cnt.item())
sym, ns = (int(x) for x in res.cpu())
n_kept, total, need, g_sym = (int(x) for x in g_res.cpu())
assert need <= g_cap and g_sym == sym and 0 < sym <= out_cap and torch.equal(out[:sym], g_out[:sym]), (sym, g_sym, need)
plan.status()

WINDOWS = {"symbols_8_8": (8, 8, MERGE), "symbols_40_40": (40, 40, MERGE), "texts_1_1": (1, 1, TEXTS | MERGE), "texts_0_0": (0, 0, TEXTS | MERGE)}
fns = {"a_scan_ordered": ordered, "g_grep_gather": grep(True), "g0_grep_no_gather": grep(False)}
shape = {}
for name, (b, a, f) in WINDOWS.items():
    fns["b_context_" + name] = context(b, a, f)
    fns["b0_context_no_gather_" + name] = context(b, a, f, gather=False)
    fns["c_fused_" + name] = fused(b, a, f)
    ordered()
    context(b, a, f)()
    torch.cuda.synchronize()
    sym, ns = (int(x) for x in res.cpu())
    assert 0 < sym <= out_cap and 1 < ns < records
    shape[name] = {"n_snippets": ns, "out_symbols": sym}
ordered()                                                             # (b) reads the records of (a): leave them in place
for fn in list(fns.values()) * 2:                                     # warm-up of every shape
    fn()
ordered()
steps = max(5, int(args.window * 1e3 / max(timed(fns["c_fused_texts_1_1"], 5), 1e-3)))
rounds = {k: [] for k in fns}
for _ in range(args.rounds):                                          # alternating, so that drift hits all alike
    for k, fn in fns.items():
        if k.startswith("b"):
            ordered()                                                 # (the fused call in front rewrote the records: the same ones)
        rounds[k].append(timed(fn, steps))
plan.status()
med = {k: float(np.median(v)) for k, v in rounds.items()}
gather = {name: med["b_context_" + name] - med["b0_context_no_gather_" + name] for name in WINDOWS}
case = {"keywords": args.keywords, "text_bytes": n, "kernel": int(plan.info.kernel), "line_symbols": args.line, "n_texts": n_texts, "records": records,
        "steps_per_round": steps, "tmp_bytes_ordered": int(to), "tmp_bytes_context": int(tc), "tmp_bytes_scan_context": int(tf), "windows": shape,
        "ms": med, "rounds_ms": rounds,
        "c_minus_a_ms": {name: med["c_fused_" + name] - med["a_scan_ordered"] for name in WINDOWS},
        "context_gather_ms": gather,
        "context_gather_bytes_per_s": {name: shape[name]["out_symbols"] / (gather[name] * 1e-3) for name in WINDOWS},
        "grep_gather_ms": med["g_grep_gather"] - med["g0_grep_no_gather"], "grep_gather_bytes": g_sym,
        "grep_gather_bytes_per_s": g_sym / ((med["g_grep_gather"] - med["g0_grep_no_gather"]) * 1e-3)}
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_context.py: ms per call, medians of %d rounds of about %.2f s each, all calls alternating" % (
            args.rounds, args.window), "device": torch.cuda.get_device_name(0), "case": case}, f, indent=1)
        f.write("\n")
