"""Experiment driver: what the TEMPLATES passes cost beside the ordered scan that runs in front of them.
The text is the novel of tests/golden repeated to --mib MiB with one social-security-shaped number, one date and one
signature planted per copy; the templates are `\\d{3}-\\d{2}-\\d{4}` (its seed `-` is frequent: the case to watch),
`[A-Z][a-z]{2}\\.\\sDalloway`, `20\\d\\d-[01]\\d-[0-3]\\d` and the hex signature `45 3? ?? ?3 [41-4F] 7E`, cut at
k = 0 (TemplateSet.from_templates).  Per template set -- all four, and the first alone -- this times, in one process,
on one plan and one text, alternating,
  (a) acm_gpu_scan_ordered_device alone, into the record room the count pass found;
  (b) the TEMPLATES passes alone: acm_gpu_templates_records_device over (a)'s records, the count on the device;
  (c) acm_gpu_scan_templates_device, which is (a) followed by (b) in one call.
Every round gives each figure at least --window seconds of work, timed between two device events; ms per call,
the median of the rounds and their spread (max - min over the median).  Before anything is timed (c)'s matches
are compared with (b)'s, and both with Python's `re` on the first copy of the novel.  Prints one JSON line per set
and writes them to --out if given (profiles/templates.json is one such run)."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import RECORD_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--mib", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.5, help="seconds of work per figure and round")
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


with open(os.path.join(ROOT, "tests", "golden", "mrs_dalloway.txt"), "rb") as f:
    novel = f.read() + b" 078-05-1120 2024-02-29 " + bytes([0x45, 0x3A, 0x00, 0xC3, 0x41, 0x7E]) + b"\n"
n = args.mib << 20
host = (novel * (n // len(novel) + 1))[:n]
text = torch.from_numpy(np.frombuffer(host, np.uint8).copy()).to(dev)
PATTERNS = [rb"\d{3}-\d{2}-\d{4}", rb"[A-Z][a-z]{2}\.\sDalloway", rb"20\d\d-[01]\d-[0-3]\d", rb"\x45[\x30-\x3f].[\x03\x13\x23\x33\x43\x53\x63\x73\x83\x93\xa3\xb3\xc3\xd3\xe3\xf3][\x41-\x4f]\x7e"]
TEMPLATES = [acm.template(PATTERNS[0].decode()), acm.template(PATTERNS[1].decode()), acm.template(PATTERNS[2].decode()),
             acm.hex_template("45 3? ?? ?3 [41-4F] 7E")]
L = acm.lib()
cases = []
for name, pick in (("all four", [0, 1, 2, 3]), ("ddd-dd-dddd alone", [0])):
    m = acm.Machine(1)
    tset = acm.TemplateSet.from_templates(m, [TEMPLATES[i] for i in pick], 0)
    plan = m.plan(0)
    T = plan.templates_create(tset)
    cap = int(plan.count(text, n).item()) + 16
    records = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    _, _, tmp_a = plan.scan_ordered(text, n, records=records, count=count)
    _, _, need = plan.templates_records(records, cap, T, text, n, count=count, out_capacity=0)     # the count alone
    out_cap = int(need.item()) + 16
    out_b = torch.empty((out_cap, 2), dtype=torch.int64, device=dev)
    dist_b = torch.empty(out_cap, dtype=torch.int32, device=dev)
    cnt_b = torch.zeros(1, dtype=torch.int64, device=dev)
    out_c, dist_c = torch.empty_like(out_b), torch.empty_like(dist_b)
    tb = L.acm_gpu_templates_tmp_bytes(plan.h, T.h, cap, out_cap, 0)
    tmp_b = torch.empty(tb, dtype=torch.uint8, device=dev)
    st = plan._stream()
    state = {"tmp_c": None, "res_c": None}

    def ordered():
        plan.scan_ordered(text, n, records=records, count=count, tmp=tmp_a)

    def passes():
        rc = L.acm_gpu_templates_records_device(plan.h, T.h, records.data_ptr(), cap, count.data_ptr(), text.data_ptr(), n, 0, None, 0, out_b.data_ptr(),
                                                dist_b.data_ptr(), out_cap, cnt_b.data_ptr(), tmp_b.data_ptr(), tb, st)
        assert rc == 0, rc

    def fused():
        _, _, c, f, state["tmp_c"] = plan.scan_templates(text, T, n_symbols=n, capacity=cap, out=out_c, dist=dist_c, out_capacity=out_cap, tmp=state["tmp_c"])
        state["res_c"] = (c, f)

    # ---- the calls agree with each other and with `re` on the first copy before anything is timed
    ordered(), passes(), fused()
    torch.cuda.synchronize()
    n_rec, n_b, n_c = int(count.item()), int(cnt_b.item()), int(state["res_c"][0].item())
    assert n_rec <= cap and int(state["res_c"][1].item()) == n_rec and n_b == n_c <= out_cap, (n_rec, cap, n_b, n_c, out_cap)
    assert torch.equal(out_b[:n_b], out_c[:n_c]) and torch.equal(dist_b[:n_b], dist_c[:n_c])
    got = np.frombuffer(out_b[:n_b].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
    head = host[:len(novel)]
    want = sorted(((mt.start() + len(TEMPLATES[i]) - 1, -len(TEMPLATES[i]), w) for w, i in enumerate(pick)
                   for mt in re.finditer(b"(?=(" + PATTERNS[i] + b"))", head, re.DOTALL)))
    below = got[got["end_pos"] < len(novel)]
    assert [(int(r["end_pos"]), -int(r["length"]), int(r["keyword_id"])) for r in below] == want, "the first copy of the novel"
    plan.status()
    fns = {"a_scan_ordered": ordered, "b_templates_passes": passes, "c_scan_templates": fused}
    for fn in list(fns.values()) * 2:                                 # warm-up of every shape
        fn()
    steps = {k: max(3, int(np.ceil(args.window * 1e3 / max(timed(fn, 3), 1e-3)))) for k, fn in fns.items()}
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):                                      # alternating, so that drift hits all alike
        for k, fn in fns.items():
            rounds[k].append(timed(fn, steps[k]))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
    case = {"what": "tools/exp_templates.py: ms per call, medians of %d rounds of at least %.1f s per figure, (a) (b) (c) alternating; spread = "
                    "(max - min) / median of the rounds; class bitmaps read from global memory" % (args.rounds, args.window),
            "set_name": name, "device": torch.cuda.get_device_name(0), "text_bytes": int(n), "templates": [PATTERNS[i].decode("latin-1") for i in pick],
            "keywords": [bytes(m.keyword(i)[0]).decode("latin-1") for i in range(m.nb_keywords)], "kernel": int(plan.info.kernel), "set": T.info(),
            "records": n_rec, "matches": n_b, "checked_matches": len(want), "templates_tmp_bytes": int(tb), "steps_per_round": steps, "ms": med,
            "spread": spread, "rounds_ms": rounds, "records_per_s_in_b": n_rec / (med["b_templates_passes"] * 1e-3),
            "b_share_of_c": med["b_templates_passes"] / med["c_scan_templates"]}
    print(json.dumps(case), flush=True)
    cases.append(case)
    T.close()
    plan.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")
