"""Experiment driver: what the EDIT passes cost beside the ordered scan in front of them and beside the APPROX
passes over the same records (tools/exp_approx.py's workload: the text shape of config 2, --targets targets of
--length symbols taken from the text itself and cut at --k into k + 1 pieces that join the dictionary).  This
times, in one process, on one plan and one text, alternating,
  (a) acm_gpu_scan_ordered_device alone, into the record room the count pass found;
  (b) the APPROX passes alone (acm_gpu_approx_records_device) over (a)'s records;
  (c) the EDIT passes alone (acm_gpu_edit_records_device) over the same records, once per --tiles entry
      (ACM_GPU_EDIT_TILE is read at every call);
  (d) acm_gpu_scan_edit_device, which is (a) followed by (c) in one call, at the default tile.
Every round gives each figure at least --window seconds of work, timed between two device events; ms per call,
the median of the rounds and their spread (max - min over the median).  Before anything is timed (d)'s matches
are compared with (c)'s at every tile, and with the definition in Python (tests/edit_cases.py, without its seed
condition: the cuts are canonical) over the text's first --check-kib KiB, where the targets are taken from.
Prints one JSON line and writes it to --out if given (profiles/edit.json is one such run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import RECORD_DTYPE
from tests.edit_cases import edits

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--targets", type=int, default=1000)
ap.add_argument("--k", type=int, default=1)
ap.add_argument("--length", type=int, default=8)
ap.add_argument("--tiles", default="64,256,1024,4096", help="ACM_GPU_EDIT_TILE values to time (c) at")
ap.add_argument("--check-kib", type=int, default=32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.5, help="seconds of work per figure and round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
tiles = [int(t) for t in args.tiles.split(",")]
os.environ.pop("ACM_GPU_EDIT_TILE", None)


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
aset.check_edit()
plan = m.plan(0)
A = plan.approx_create(aset)
cap = int(plan.count(text, n).item()) + 16
records = torch.empty((cap, 2), dtype=torch.int64, device=dev)
count = torch.zeros(1, dtype=torch.int64, device=dev)
_, _, tmp_a = plan.scan_ordered(text, n, records=records, count=count)
_, _, need = plan.edit_records(records, cap, A, text, n, count=count, out_capacity=0)       # the count alone
out_cap = int(need.item()) + 16
out_c = torch.empty((out_cap, 2), dtype=torch.int64, device=dev)
dist_c = torch.empty(out_cap, dtype=torch.int32, device=dev)
cnt_c = torch.zeros(1, dtype=torch.int64, device=dev)
cnt_b = torch.zeros(1, dtype=torch.int64, device=dev)
out_b, dist_b = torch.empty_like(out_c), torch.empty_like(dist_c)
out_d, dist_d = torch.empty_like(out_c), torch.empty_like(dist_c)
tmp_d = None
L = acm.lib()
tb = max(L.acm_gpu_edit_tmp_bytes(plan.h, A.h, cap, out_cap, 0), L.acm_gpu_approx_tmp_bytes(plan.h, A.h, cap, out_cap, 0))
tmp_c = torch.empty(tb, dtype=torch.uint8, device=dev)
st = plan._stream()


def ordered():
    plan.scan_ordered(text, n, records=records, count=count, tmp=tmp_a)


def approx_passes():
    rc = L.acm_gpu_approx_records_device(plan.h, A.h, records.data_ptr(), cap, count.data_ptr(), text.data_ptr(), n, 0, None, 0, out_b.data_ptr(),
                                         dist_b.data_ptr(), out_cap, cnt_b.data_ptr(), tmp_c.data_ptr(), tb, st)
    assert rc == 0, rc


def edit_passes(tile=None):
    if tile is None:
        os.environ.pop("ACM_GPU_EDIT_TILE", None)
    else:
        os.environ["ACM_GPU_EDIT_TILE"] = str(tile)
    rc = L.acm_gpu_edit_records_device(plan.h, A.h, records.data_ptr(), cap, count.data_ptr(), text.data_ptr(), n, 0, None, 0, out_c.data_ptr(),
                                       dist_c.data_ptr(), out_cap, cnt_c.data_ptr(), tmp_c.data_ptr(), tb, st)
    assert rc == 0, rc


def fused():
    global tmp_d, res_d
    os.environ.pop("ACM_GPU_EDIT_TILE", None)
    _, _, c, f, tmp_d = plan.scan_edit(text, A, n_symbols=n, capacity=cap, out=out_d, dist=dist_d, out_capacity=out_cap, tmp=tmp_d)
    res_d = (c, f)


# ---- the calls agree with each other and with the text before anything is timed
ordered(), fused()
torch.cuda.synchronize()
n_rec, n_d = int(count.item()), int(res_d[0].item())
assert n_rec <= cap and int(res_d[1].item()) == n_rec and n_d <= out_cap, (n_rec, cap, n_d, out_cap)
for tile in [None] + tiles:
    edit_passes(tile)
    torch.cuda.synchronize()
    assert int(cnt_c.item()) == n_d and torch.equal(out_c[:n_d], out_d[:n_d]) and torch.equal(dist_c[:n_d], dist_d[:n_d]), tile
got = np.frombuffer(out_d[:n_d].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
got_d = dist_d[:n_d].cpu().numpy()
inside = head.size - args.length - args.k                        # (ends whose every start lies in the head)
below = got["end_pos"] < inside
want = edits(None, head, targets, [args.k] * len(targets), None, seeded=False)
keep = want[0]["end_pos"] < inside
assert np.array_equal(got[below], want[0][keep]) and np.array_equal(got_d[below].astype(np.uint32), want[1][keep]), "the head of the text"
plan.status()
approx_passes()
torch.cuda.synchronize()
n_b = int(cnt_b.item())

fns = {"a_scan_ordered": ordered, "b_approx_passes": approx_passes, "c_edit_passes": edit_passes, "d_scan_edit": fused}
for tile in tiles:
    fns["c_edit_passes_tile_%d" % tile] = (lambda t: lambda: edit_passes(t))(tile)
for fn in list(fns.values()) * 2:                                 # warm-up of every shape
    fn()
steps = {k: max(3, int(np.ceil(args.window * 1e3 / max(timed(fn, 3), 1e-3)))) for k, fn in fns.items()}
rounds = {k: [] for k in fns}
for _ in range(args.rounds):                                      # alternating, so that drift hits all alike
    for k, fn in fns.items():
        rounds[k].append(timed(fn, steps[k]))
med = {k: float(np.median(v)) for k, v in rounds.items()}
spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
case = {"what": "tools/exp_edit.py: ms per call, medians of %d rounds of at least %.1f s per figure, alternating; spread = (max - min) / median of the "
                "rounds" % (args.rounds, args.window),
        "device": torch.cuda.get_device_name(0), "text_bytes": int(n), "targets": args.targets, "length": args.length, "k": args.k,
        "keywords": m.nb_keywords, "kernel": int(plan.info.kernel), "set": A.info(), "records": n_rec, "record_capacity": cap, "edit_matches": n_d,
        "edit_matches_by_distance": np.bincount(got_d).tolist(), "approx_matches": n_b, "checked_matches": int(np.count_nonzero(keep)),
        "out_capacity": out_cap, "tmp_bytes": int(tb), "steps_per_round": steps, "ms": med, "spread": spread, "rounds_ms": rounds,
        "records_per_s_in_c": n_rec / (med["c_edit_passes"] * 1e-3), "c_over_b": med["c_edit_passes"] / med["b_approx_passes"],
        "c_over_a": med["c_edit_passes"] / med["a_scan_ordered"]}
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(case, f, indent=1)
        f.write("\n")
