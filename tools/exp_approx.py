"""Experiment driver: what the APPROX passes cost beside the ordered scan that runs in front of them.
On the text shape of config 2 (bench.py: 1,000 synthetic ASCII keywords, --mib MiB of synthetic text generated on
the device) 1,000 targets of eight symbols are taken from the text itself and cut at k = 1 into two pieces of four
(ApproxSet.from_targets: the pieces join the dictionary, so the plan holds about 3,000 keywords).  This times, in
one process, on one plan and one text, alternating,
  (a) acm_gpu_scan_ordered_device alone, into the record room the count pass found;
  (b) the APPROX passes alone: acm_gpu_approx_records_device over (a)'s records, the count on the device;
  (c) acm_gpu_scan_approx_device, which is (a) followed by (b) in one call.
Every round gives each figure at least --window seconds of work, timed between two device events; ms per call,
the median of the rounds and their spread (max - min over the median).  Before anything is timed (c)'s matches
are compared with (b)'s, and both with a numpy Hamming scan of the text's first --check-kib KiB, where the targets
are taken from.  Prints one JSON line and writes it to --out if given (profiles/approx.json is one such run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import RECORD_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--targets", type=int, default=1000)
ap.add_argument("--k", type=int, default=1)
ap.add_argument("--length", type=int, default=8)
ap.add_argument("--check-kib", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=1.0, help="seconds of work per figure and round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)


def timed(fn, steps):
    """ms per call between two device events on the stream the calls are queued on"""
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return begin.elapsed_time(end) / steps


kd, ko = acm.synth.keywords(1000, sym_bytes=1, vocab=32768)
n = args.mib << 20
text = acm.synth.device_text(n, kd, ko, begin=0, sym_bytes=1, vocab=32768, device=dev)
head = text[:args.check_kib << 10].cpu().numpy()
rng = np.random.default_rng(1975)
starts = rng.integers(0, head.size - args.length, size=args.targets)
targets = [head[s:s + args.length].copy() for s in starts]
m = acm.Machine(1)
m.add_keywords_packed(kd, ko, ids_as_values=True)
aset = acm.ApproxSet.from_targets(m, targets, args.k)
plan = m.plan(0)
A = plan.approx_create(aset)
cap = int(plan.count(text, n).item()) + 16
records = torch.empty((cap, 2), dtype=torch.int64, device=dev)
count = torch.zeros(1, dtype=torch.int64, device=dev)
_, _, tmp_a = plan.scan_ordered(text, n, records=records, count=count)
_, _, need = plan.approx_records(records, cap, A, text, n, count=count, out_capacity=0)     # the count alone
out_cap = int(need.item()) + 16
out_b = torch.empty((out_cap, 2), dtype=torch.int64, device=dev)
dist_b = torch.empty(out_cap, dtype=torch.int32, device=dev)
cnt_b = torch.zeros(1, dtype=torch.int64, device=dev)
out_c, dist_c = torch.empty_like(out_b), torch.empty_like(dist_b)
tmp_c = None
L = acm.lib()
tb = L.acm_gpu_approx_tmp_bytes(plan.h, A.h, cap, out_cap, 0)
tmp_b = torch.empty(tb, dtype=torch.uint8, device=dev)
st = plan._stream()


def ordered():
    plan.scan_ordered(text, n, records=records, count=count, tmp=tmp_a)


def passes():
    rc = L.acm_gpu_approx_records_device(plan.h, A.h, records.data_ptr(), cap, count.data_ptr(), text.data_ptr(), n, 0, None, 0, out_b.data_ptr(),
                                         dist_b.data_ptr(), out_cap, cnt_b.data_ptr(), tmp_b.data_ptr(), tb, st)
    assert rc == 0, rc


def fused():
    global tmp_c, res_c
    _, _, c, f, tmp_c = plan.scan_approx(text, A, n_symbols=n, capacity=cap, out=out_c, dist=dist_c, out_capacity=out_cap, tmp=tmp_c)
    res_c = (c, f)


# ---- the calls agree with each other and with the text before anything is timed
ordered(), passes(), fused()
torch.cuda.synchronize()
n_rec, n_b, n_c = int(count.item()), int(cnt_b.item()), int(res_c[0].item())
assert n_rec <= cap and int(res_c[1].item()) == n_rec and n_b == n_c <= out_cap, (n_rec, cap, n_b, n_c, out_cap)
assert torch.equal(out_b[:n_b], out_c[:n_c]) and torch.equal(dist_b[:n_b], dist_c[:n_c])
got = np.frombuffer(out_b[:n_b].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
got_d = dist_b[:n_b].cpu().numpy()
below = got["end_pos"] < head.size
want = []
for w, t in enumerate(targets):
    d = np.count_nonzero(np.lib.stride_tricks.sliding_window_view(head, t.size) != t, axis=1)
    for s in np.nonzero(d <= args.k)[0]:
        want.append((int(s) + t.size - 1, t.size, w, int(d[s])))
want.sort(key=lambda r: (r[0], -r[1], r[2]))
assert [(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"]), int(x)) for r, x in zip(got[below], got_d[below])] == want, "the head of the text"
plan.status()

fns = {"a_scan_ordered": ordered, "b_approx_passes": passes, "c_scan_approx": fused}
for fn in list(fns.values()) * 2:                                 # warm-up of every shape
    fn()
steps = {k: max(3, int(np.ceil(args.window * 1e3 / max(timed(fn, 3), 1e-3)))) for k, fn in fns.items()}
rounds = {k: [] for k in fns}
for _ in range(args.rounds):                                      # alternating, so that drift hits all alike
    for k, fn in fns.items():
        rounds[k].append(timed(fn, steps[k]))
med = {k: float(np.median(v)) for k, v in rounds.items()}
spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
info = A.info()
case = {"what": "tools/exp_approx.py: ms per call, medians of %d rounds of at least %.1f s per figure, (a) (b) (c) alternating; spread = (max - min) / "
                "median of the rounds" % (args.rounds, args.window),
        "device": torch.cuda.get_device_name(0), "text_bytes": int(n), "targets": args.targets, "length": args.length, "k": args.k,
        "keywords": m.nb_keywords, "kernel": int(plan.info.kernel), "set": info, "records": n_rec, "record_capacity": cap, "matches": n_b,
        "matches_with_mismatches": int(np.count_nonzero(got_d)), "checked_matches": len(want), "out_capacity": out_cap, "approx_tmp_bytes": int(tb),
        "steps_per_round": steps, "ms": med, "spread": spread, "rounds_ms": rounds,
        "records_per_s_in_b": n_rec / (med["b_approx_passes"] * 1e-3), "b_over_a": med["b_approx_passes"] / med["a_scan_ordered"]}
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(case, f, indent=1)
        f.write("\n")
