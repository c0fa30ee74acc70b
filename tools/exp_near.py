"""Experiment driver: what the NEAR join costs per record, beside the CHAINS join of the same records.
One workload on one plan and one text, in one process, alternating: config 2's text shape and dictionary (--mib
MiB, 1,000 keywords, about one record per 2 KiB), --groups NEAR groups of two to four random keywords of the
dictionary (need = all), once per width of --widths.  The records are those of one acm_gpu_scan_ordered_device
call; they stay on the device and every figure is a join of them alone:
  (a) acm_gpu_near_records_device, per width, per ACM_GPU_NEAR_TILE of --tiles and per ACM_GPU_NEAR_COOP of --coops
      (both read at every call; `off` is 2,147,483,647);
  (b) acm_gpu_chains_records_device -- the yardstick, code that was there before NEAR -- with the two-term
      ordered chains `A gap(0, width) B` of every group's first two keywords.
Every round gives each figure at least --window seconds of work, timed between two device events; ms per call,
the median of the rounds and their spread (max - min over the median), and ns per record.  Before anything is
timed the matches of every TILE and COOP value are compared with each other, and those that end in the text's first
--check-kib KiB with the sequential pass on the host (acm_near_records) over the records there.
The walk kernel's share of the join is not taken here: run the tool once more with `--rounds 1 --window 0.2`
under `rocprofv3 --kernel-trace --stats` and read near_walk_kernel against the other kernels of the join in its
*_kernel_stats.csv.
Prints one JSON line and writes it to --out if given (profiles/near.json is one such run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import RECORD_DTYPE, lib

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--groups", type=int, default=64)
ap.add_argument("--widths", default="32,1024,1048576")
ap.add_argument("--tiles", default="64,256,1024,4096")
ap.add_argument("--coops", default="0,64,off")
ap.add_argument("--check-kib", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--window", type=float, default=0.5, help="seconds of work per figure and round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
widths = [int(w) for w in args.widths.split(",")]
coops = [c for c in args.coops.split(",")]
shapes = [(t, c) for t in args.tiles.split(",") for c in coops]
OFF = "2147483647"
L = lib()


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


def set_shape(shape):
    os.environ["ACM_GPU_NEAR_TILE"], coop = shape
    os.environ["ACM_GPU_NEAR_COOP"] = OFF if coop == "off" else coop


def random_groups(rng, n_groups, n_keywords):
    """groups of two to four distinct keywords, the sizes in turn"""
    return [[int(k) for k in rng.choice(n_keywords, size=2 + g % 3, replace=False)] for g in range(n_groups)]


kd, ko = acm.synth.keywords(1000, sym_bytes=1, vocab=32768)
n = args.mib << 20
text = acm.synth.device_text(n, kd, ko, begin=0, sym_bytes=1, vocab=32768, device=dev)
m = acm.Machine(1)
m.add_keywords_packed(kd, ko, ids_as_values=True)
plan = m.plan(0)
cap = int(plan.count(text, n).item()) + 16
records = torch.empty((cap, 2), dtype=torch.int64, device=dev)
count = torch.zeros(1, dtype=torch.int64, device=dev)
plan.scan_ordered(text, n, records=records, count=count)
torch.cuda.synchronize()
n_rec = int(count.item())
head = min(args.check_kib << 10, n)
rec_host = np.frombuffer(records[:n_rec].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
rec_head = rec_host[rec_host["end_pos"] < head]
ids = random_groups(np.random.default_rng(1975), args.groups, m.nb_keywords)
stream = plan._stream()
fns, facts, keep = {}, {}, []
for width in widths:
    group_list = [(g, width, 0) for g in ids]
    chain_list = [[(g[0], 0, 0), (g[1], 0, width)] for g in ids]
    S, Ch = plan.near(group_list), plan.chains_create(chain_list)
    out_cap = cap * max(S.info()["max_postings"], Ch.info()["max_last_postings"])
    out = torch.empty((max(out_cap, 1), 2), dtype=torch.int64, device=dev)
    res = torch.zeros(2, dtype=torch.int64, device=dev)
    tb_near, tb_chains = L.acm_gpu_near_tmp_bytes(plan.h, S.h, cap, 0), L.acm_gpu_chains_tmp_bytes(plan.h, Ch.h, cap, 0)
    tmp = torch.empty(max(tb_near, tb_chains), dtype=torch.uint8, device=dev)
    keep += [S, Ch, out, res, tmp]

    def near_join(shape, S=S, out=out, res=res, tmp=tmp, out_cap=out_cap, tb=tb_near):
        set_shape(shape)
        rc = L.acm_gpu_near_records_device(plan.h, S.h, records.data_ptr(), cap, count.data_ptr(), n, 0, None, 0, out.data_ptr(), out_cap, res.data_ptr(),
                                           tmp.data_ptr(), tb, stream)
        assert rc == 0, rc

    def chains_join(Ch=Ch, out=out, res=res, tmp=tmp, out_cap=out_cap, tb=tb_chains):
        rc = L.acm_gpu_chains_records_device(plan.h, Ch.h, records.data_ptr(), cap, count.data_ptr(), n, 0, None, 0, out.data_ptr(), out_cap,
                                             res.data_ptr() + 8, tmp.data_ptr(), tb, stream)
        assert rc == 0, rc
    # ---- the walk forms agree with each other and with the host's sequential pass before anything is timed
    first = None
    for shape in shapes:
        near_join(shape)
        torch.cuda.synchronize()
        n_out = int(res[0].item())
        assert n_out <= out_cap, (width, shape)
        got = out[:n_out].clone()
        if first is None:
            first = got
        assert torch.equal(got, first), (width, shape)
    got = np.frombuffer(first.cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
    want = acm.near_records(rec_head, group_list, head, n_keywords=m.nb_keywords)
    assert np.array_equal(got[got["end_pos"] < head], want), (width, "the head of the text")
    chains_join()
    torch.cuda.synchronize()
    plan.status()
    facts[width] = {"near_set": S.info(), "chains_set": Ch.info(), "near_matches": int(got.size), "checked_matches": int(want.size),
                    "chains_matches": int(res[1].item()), "out_capacity": int(out_cap), "near_tmp_bytes": int(tb_near), "chains_tmp_bytes": int(tb_chains)}
    for shape in shapes:
        fns["near_width_%d_tile_%s_coop_%s" % ((width,) + shape)] = (lambda c, f: lambda: f(c))(shape, near_join)
    fns["chains_width_%d" % width] = chains_join
for fn in list(fns.values()) * 2:                                 # warm-up of every shape
    fn()
steps = {k: max(1, int(np.ceil(args.window * 1e3 / max(timed(fn, 1), 1e-3)))) for k, fn in fns.items()}
rounds = {k: [] for k in fns}
for _ in range(args.rounds):                                      # alternating, so that drift hits all alike
    for k, fn in fns.items():
        rounds[k].append(timed(fn, steps[k]))
med = {k: float(np.median(v)) for k, v in rounds.items()}
spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
os.environ.pop("ACM_GPU_NEAR_COOP", None)
os.environ.pop("ACM_GPU_NEAR_TILE", None)
case = {"what": "tools/exp_near.py: the joins of one record set that stays on the device, ms per call, medians of %d rounds of at least %.1f s per "
                "figure, alternating; spread = (max - min) / median of the rounds; ns_per_record = ms x 1e6 / records" % (args.rounds, args.window),
        "device": torch.cuda.get_device_name(0), "widths": widths, "tiles": args.tiles.split(","), "coops": coops, "text_bytes": int(n), "keywords": m.nb_keywords,
        "kernel": int(plan.info.kernel), "groups": args.groups, "records": n_rec, "record_capacity": cap, "checked_bytes": int(head),
        "per_width": facts, "steps_per_round": steps, "ms": med, "ns_per_record": {k: v * 1e6 / max(n_rec, 1) for k, v in med.items()},
        "spread": spread, "rounds_ms": rounds}
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(case, f, indent=1)
        f.write("\n")
