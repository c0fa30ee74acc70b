"""Experiment driver: what the per-text keyword counts of a batch (acm_gpu_tally_batch_device,
csrc/dev_tally_batch.h) cost beside the nearest existing pipeline and beside the only way to get the
same answer without them, on a batch resident on the device:
  (a) acm_gpu_grep_device without a gather      -- the same window scans plus one histogram pass: one
                                                   counter per text, not the matrix;
  (b) acm_gpu_tally_batch_device                -- the text x keyword count matrix in CSR form;
  (c) acm_gpu_scan_batch_device + torch.unique  -- the ordered batch scan into a record room for the
                                                   whole buffer, then unique over text_id << 32 |
                                                   keyword_id with counts, on the device (the rows
                                                   still lack their row pointers);
for config 2's dictionary (1,000 keywords, dense kernel) and synthetic text cut into texts of 700
symbols on average (tests/batch_cases.random_cuts' rule).  The paths alternate inside one timed loop,
several rounds; every path is timed with device events around `steps` calls.  (b) is checked against
(c)'s answer before anything is timed.  Then (b) alone over the sizes of the LDS table and over R.
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "tally_batch.json"))
ap.add_argument("--log2", type=int, default=28, help="text size")
ap.add_argument("--window-log2", type=int, default=24, help="window of (a) and (b)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed round")
ap.add_argument("--no-sweep", action="store_true")
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


def random_cuts(n, mean, seed=7):
    """tests/batch_cases.random_cuts: n // mean random cut points, some doubled and tripled (empty texts)"""
    rng = np.random.default_rng(seed)
    cuts = rng.integers(0, n + 1, n // mean)
    dup = cuts[:: max(cuts.size // 50, 1)]
    return np.sort(np.concatenate([[0, 0, 0], cuts, dup, dup[::3], [n, n]])).astype(np.int64)


n = 1 << args.log2
K = 1000
kd, ko = acm.synth.keywords(K)
m = acm.Machine(1)
m.add_keywords_packed(kd, ko)
plan = m.plan(0)
text = acm.synth.device_text(n, kd, ko)
off = torch.from_numpy(random_cuts(n, 700)).cuda()
n_texts = off.numel() - 1
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
whole = int(plan.count(text, count=cnt).item())
window = min(1 << args.window_log2, n)
densest = max(int(plan.count(text[b:b + window], count=cnt).item()) for b in range(0, n, window))
capacity = densest + densest // 8 + 4096

# (c) the batch scan into room for every record of the concatenation, then unique with counts
rec = torch.empty((whole + 1024, 2), dtype=torch.int64, device="cuda")
tid = torch.empty(whole + 1024, dtype=torch.int32, device="cuda")
first = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
sb_bytes = L.acm_gpu_scan_batch_tmp_bytes(plan.h, whole + 1024, n, n_texts)
sb_tmp = torch.empty(max(sb_bytes, 16), dtype=torch.uint8, device="cuda")


def scan_batch():
    _check(L.acm_gpu_scan_batch_device(plan.h, text.data_ptr(), n, off.data_ptr(), n_texts, rec.data_ptr(), tid.data_ptr(), first.data_ptr(),
                                       whole + 1024, cnt.data_ptr(), sb_tmp.data_ptr(), sb_bytes, st), "acm_gpu_scan_batch_device")


scan_batch()
kept = int(cnt.item())
assert 0 < kept <= whole


def scan_batch_unique():
    scan_batch()
    keys = (tid[:kept].to(torch.int64) << 32) | (rec[:kept, 1] >> 32)          # (kept is known: no read-back inside the timed call)
    return torch.unique(keys, return_counts=True)


want_keys, want_counts = scan_batch_unique()
nnz = want_keys.numel()

# (b)
pair_capacity = kept
row_ptr = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
col = torch.zeros(pair_capacity, dtype=torch.int32, device="cuda")
val = torch.zeros(pair_capacity, dtype=torch.int64, device="cuda")
res = torch.zeros(4, dtype=torch.int64, device="cuda")
tb_bytes = L.acm_gpu_tally_batch_tmp_bytes(plan.h, window, capacity, pair_capacity, n, n_texts)
tb_tmp = torch.empty(tb_bytes, dtype=torch.uint8, device="cuda")


def tally_batch():
    _check(L.acm_gpu_tally_batch_device(plan.h, text.data_ptr(), n, off.data_ptr(), n_texts, window, capacity, pair_capacity, row_ptr.data_ptr(),
                                        col.data_ptr(), val.data_ptr(), res.data_ptr(), res.data_ptr() + 8, res.data_ptr() + 16,
                                        res.data_ptr() + 24, tb_tmp.data_ptr(), tb_bytes, st), "acm_gpu_tally_batch_device")


def checked():
    tally_batch()
    got = [int(x) for x in res.cpu()]
    assert got[0] == nnz and got[1] == kept and got[2] <= capacity and got[3] <= pair_capacity, (got, nnz, kept)
    rows = torch.repeat_interleave(torch.arange(n_texts, device="cuda"), row_ptr[1:] - row_ptr[:-1])
    assert torch.equal((rows << 32) | col[:nnz].to(torch.int64), want_keys) and torch.equal(val[:nnz], want_counts)
    return got


partial = checked()[3]

# (a)
hits = torch.zeros(n_texts, dtype=torch.int64, device="cuda")
keep = torch.zeros(n_texts, dtype=torch.int32, device="cuda")
out_off = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
gres = torch.zeros(4, dtype=torch.int64, device="cuda")
g_bytes = L.acm_gpu_grep_tmp_bytes(plan.h, window, capacity, n, n_texts)
g_tmp = torch.empty(g_bytes, dtype=torch.uint8, device="cuda")


def grep():
    _check(L.acm_gpu_grep_device(plan.h, text.data_ptr(), n, off.data_ptr(), n_texts, 0, window, capacity, hits.data_ptr(), keep.data_ptr(),
                                 gres.data_ptr(), gres.data_ptr() + 8, gres.data_ptr() + 16, None, 0, out_off.data_ptr(), None, g_tmp.data_ptr(),
                                 g_bytes, st), "acm_gpu_grep_device")


grep()
assert int(gres[1].item()) == kept
r, steps = measure({"a_grep": grep, "b_tally_batch": tally_batch, "c_scan_batch_unique": scan_batch_unique})
a, b, c = (r[k][0] for k in ("a_grep", "b_tally_batch", "c_scan_batch_unique"))
out = {"what": "tools/exp_tally_batch.py: ms per call, medians of %d rounds of about %.1f s each, the paths alternating, device events; "
               "(a) = acm_gpu_grep_device without a gather, (b) = acm_gpu_tally_batch_device, (c) = acm_gpu_scan_batch_device + torch.unique "
               "with counts" % (args.rounds, args.window),
       "device": torch.cuda.get_device_name(0), "keywords": K, "text_bytes": n, "texts": n_texts, "kernel": int(plan.info.kernel),
       "records_of_the_concatenation": whole, "records_of_the_batch": kept, "entries": nnz, "partial_pairs": partial, "window_symbols": window,
       "capacity_records": capacity, "pair_capacity": pair_capacity, "steps_per_round": steps, "a_grep_ms": a, "b_tally_batch_ms": b,
       "c_scan_batch_unique_ms": c, "b_over_a": b / a, "b_over_c": b / c, "rounds_ms": {k: v[1] for k, v in r.items()}}
print(json.dumps(out), flush=True)
if not args.no_sweep:
    sweep = {}
    for name, values in (("ACM_GPU_TALLY_BATCH_SLOTS", (256, 1024, 4096)), ("ACM_GPU_TALLY_BATCH_ROW", (256, 1024, 2048))):
        for v in values:
            os.environ[name] = str(v)
            got = checked()
            sweep["%s=%d" % (name, v)] = {"ms": measure({"b": tally_batch})[0]["b"][0], "partial_pairs": got[3]}
            print(name, v, sweep["%s=%d" % (name, v)], flush=True)
        os.environ.pop(name)
    out["sweep_b_tally_batch"] = sweep
plan.status()
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
