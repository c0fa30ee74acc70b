"""Experiment driver: what the CHAINS passes cost beside the ordered scan in front of them, and where the level
kernel's two walk forms cross.  Two workloads, each on one plan and one text, in one process, alternating:
  sparse: config 2's text shape and dictionary (--mib MiB, 1,000 keywords, about one record per 4 KiB), --chains
          chains of two and three terms over random keywords of the dictionary (two in three have two terms);
  dense:  the first --dense-mib MiB of the same text under the 26 one-letter keywords (a record at every
          symbol, so a window of gap_max symbols holds gap_max records), --dense-chains chains.
Per workload this times
  (a) acm_gpu_scan_ordered_device alone, into the record room the count pass found;
  (b) acm_gpu_scan_chains_device, which is (a) followed by the passes, once per gap_max of --gaps (every gap is
      0 .. gap_max) and per ACM_GPU_CHAINS_COOP of --coops (read at every call; `off` is 1,000,000,000).
Every round gives each figure at least --window seconds of work, timed between two device events; ms per call,
the median of the rounds and their spread (max - min over the median).  Before anything is timed the matches of
every COOP value are compared with each other, and those that end in the text's first --check-kib KiB with the
sequential pass on the host (acm_chains_records) over the ordered scan's records there.
Prints one JSON line and writes it to --out if given (profiles/chains.json is one such run)."""
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
ap.add_argument("--chains", type=int, default=300)
ap.add_argument("--dense-mib", type=int, default=4)
ap.add_argument("--dense-chains", type=int, default=24)
ap.add_argument("--gaps", default="16,256,4096")
ap.add_argument("--coops", default="0,64,off")
ap.add_argument("--check-kib", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--window", type=float, default=0.5, help="seconds of work per figure and round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
gaps = [int(g) for g in args.gaps.split(",")]
coops = [c for c in args.coops.split(",")]
OFF = "1000000000"


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


def set_coop(coop):
    os.environ["ACM_GPU_CHAINS_COOP"] = OFF if coop == "off" else coop


def random_chains(rng, n_chains, n_keywords, gap_max):
    out = []
    for c in range(n_chains):
        terms = 2 if c % 3 else 3
        out.append([(int(rng.integers(0, n_keywords)), 0, gap_max if j else 0) for j in range(terms)])
    return out


def workload(name, m, text, n, n_chains):
    plan = m.plan(0)
    cap = int(plan.count(text, n).item()) + 16
    records = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    _, _, tmp_a = plan.scan_ordered(text, n, records=records, count=count)
    torch.cuda.synchronize()
    n_rec = int(count.item())
    head = args.check_kib << 10
    rec_host = np.frombuffer(records[:n_rec].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
    rec_head = rec_host[rec_host["end_pos"] < head]
    fns = {"a_scan_ordered": lambda: plan.scan_ordered(text, n, records=records, count=count, tmp=tmp_a)}
    sets, facts = {}, {}
    for gap in gaps:
        chain_list = random_chains(np.random.default_rng(1975 + gap), n_chains, m.nb_keywords, gap)
        S = plan.chains_create(chain_list)
        info = S.info()
        out_cap = cap * info["max_last_postings"]
        state = {"out": torch.empty((max(out_cap, 1), 2), dtype=torch.int64, device=dev), "tmp": None}
        sets[gap] = (S, state)

        def fused(coop, S=S, state=state, out_cap=out_cap):
            set_coop(coop)
            _, c, f, state["tmp"] = plan.scan_chains(text, S, n_symbols=n, capacity=cap, out=state["out"], out_capacity=out_cap, tmp=state["tmp"])
            state["res"] = (c, f)
        # ---- the walk forms agree with each other and with the host's sequential pass before anything is timed
        first = None
        for coop in coops:
            fused(coop)
            torch.cuda.synchronize()
            n_out = int(state["res"][0].item())
            assert int(state["res"][1].item()) == n_rec and n_out <= out_cap, (name, gap, coop)
            got = state["out"][:n_out].clone()
            if first is None:
                first = got
            assert torch.equal(got, first), (name, gap, coop)
        got = np.frombuffer(first.cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
        want = acm.chains_records(rec_head, chain_list, head, n_keywords=m.nb_keywords)
        assert np.array_equal(got[got["end_pos"] < head], want), (name, gap, "the head of the text")
        plan.status()
        facts[gap] = {"set": info, "matches": int(got.size), "checked_matches": int(want.size), "out_capacity": int(out_cap),
                      "tmp_bytes": int(state["tmp"].numel())}
        for coop in coops:
            fns["b_scan_chains_gap_%d_coop_%s" % (gap, coop)] = (lambda c, f: lambda: f(c))(coop, fused)
    for fn in list(fns.values()) * 2:                             # warm-up of every shape
        fn()
    steps = {k: max(1, int(np.ceil(args.window * 1e3 / max(timed(fn, 1), 1e-3)))) for k, fn in fns.items()}
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):                                  # alternating, so that drift hits all alike
        for k, fn in fns.items():
            rounds[k].append(timed(fn, steps[k]))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
    for S, _ in sets.values():
        S.close()
    return {"text_bytes": int(n), "keywords": m.nb_keywords, "kernel": int(plan.info.kernel), "chains": n_chains, "records": n_rec,
            "record_capacity": cap, "per_gap": facts, "steps_per_round": steps, "ms": med, "spread": spread, "rounds_ms": rounds,
            "passes_ms": {k: v - med["a_scan_ordered"] for k, v in med.items() if k != "a_scan_ordered"}}


kd, ko = acm.synth.keywords(1000, sym_bytes=1, vocab=32768)
n = args.mib << 20
text = acm.synth.device_text(n, kd, ko, begin=0, sym_bytes=1, vocab=32768, device=dev)
sparse = acm.Machine(1)
sparse.add_keywords_packed(kd, ko, ids_as_values=True)
dense = acm.Machine(1)
for letter in range(26):
    dense.add_keyword(bytes([ord("a") + letter]))
case = {"what": "tools/exp_chains.py: ms per call, medians of %d rounds of at least %.1f s per figure, alternating; spread = (max - min) / median of the "
                "rounds; passes_ms = a fused call's median minus the ordered scan's" % (args.rounds, args.window),
        "device": torch.cuda.get_device_name(0), "gaps": gaps, "coops": coops,
        "sparse": workload("sparse", sparse, text, n, args.chains),
        "dense": workload("dense", dense, text, args.dense_mib << 20, args.dense_chains)}
os.environ.pop("ACM_GPU_CHAINS_COOP", None)
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(case, f, indent=1)
        f.write("\n")
