"""Experiment driver: what search-and-replace costs beside the selection it runs behind, and beside a
plain copy.  acm_gpu_scan_replace_device is acm_gpu_scan_select_device plus the passes of
csrc/dev_replace.h.  This times, in one process and on one build, on a text resident on the device,
  (a) acm_gpu_scan_select_device of the buffer;
  (b) acm_gpu_scan_replace_device of the same buffer into the same record room;
  (c) a plain device-to-device copy of the buffer on the same stream -- the yardstick of the output
      pass, which reads and writes every byte once as the copy does,
for the 1,000-keyword synthetic dictionary on 1 Gi byte symbols with a table that changes lengths
(replacement = keyword reversed plus one symbol), and for one dense case: the letters a-z as keywords
on 64 Mi symbols, where every symbol is a match.  (a), (b) and (c) alternate inside one timed loop,
several rounds, every round ending in a device synchronise; ms per call, medians.  Prints one JSON
line per case and writes them to --out (profiles/replace.json unless another is given)."""
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
from aho_corasick_1975_amd.binding import lib, _check, replacement_table

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "replace.json"))
ap.add_argument("--log2", type=int, default=30)
ap.add_argument("--dense-log2", type=int, default=26)
ap.add_argument("--keywords", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(name, machine, text, n, table):
    plan = machine.plan(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = torch.zeros(2, dtype=torch.int64, device="cuda")
    cap = int(plan.count(text).item()) + 4096
    assert cap < 1 << 31, "more matches than a selection takes"
    rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    data, off, nk = replacement_table(table, 1)
    d_data = torch.from_numpy(data).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    longest = int(np.diff(off.astype(np.int64)).max())
    ts = L.acm_gpu_scan_select_tmp_bytes(plan.h, cap, n)
    tr = L.acm_gpu_scan_replace_tmp_bytes(plan.h, cap, n)
    tmp = torch.empty(max(ts, tr), dtype=torch.uint8, device="cuda")

    def select():
        _check(L.acm_gpu_scan_select_device(plan.h, text.data_ptr(), n, 0, rec.data_ptr(), cap, res.data_ptr(), tmp.data_ptr(), ts, st),
               "acm_gpu_scan_select_device")

    select()
    torch.cuda.synchronize()
    selected = int(res[0].item())
    assert 0 < selected <= cap
    out_cap = n + selected * max(longest - 1, 0) + 16
    out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
    copy_to = torch.empty(n, dtype=torch.uint8, device="cuda")

    def replace():
        _check(L.acm_gpu_scan_replace_device(plan.h, text.data_ptr(), n, 0, rec.data_ptr(), cap, res.data_ptr(), d_data.data_ptr(), d_off.data_ptr(),
                                             nk, out.data_ptr(), out_cap, res.data_ptr() + 8, None, tmp.data_ptr(), tr, st),
               "acm_gpu_scan_replace_device")

    def copy():
        copy_to.copy_(text[:n])

    for fn in (replace, select, copy, replace):                    # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    count, out_symbols = (int(x) for x in res.cpu())
    assert count == selected and 0 < out_symbols <= out_cap
    plan.status()
    steps = max(3, int(args.window * 1e3 / max(timed(replace, 3), 1e-3)))
    a, b, c = [], [], []
    for _ in range(args.rounds):                                   # alternating, so that drift hits all alike
        a.append(timed(select, steps))
        b.append(timed(replace, steps))
        c.append(timed(copy, steps))
    am, bm, cm = (float(np.median(x)) for x in (a, b, c))
    case = {"case": name, "keywords": nk, "text_bytes": n, "kernel": int(plan.info.kernel), "matches": cap - 4096, "selected": selected,
            "out_symbols": out_symbols, "steps_per_round": steps, "tmp_bytes_select": int(ts), "tmp_bytes_replace": int(tr),
            "a_scan_select_ms": am, "a_rounds_ms": a, "b_scan_replace_ms": bm, "b_rounds_ms": b, "c_copy_ms": cm, "c_rounds_ms": c,
            "b_minus_a_ms": bm - am, "b_minus_a_over_c": (bm - am) / cm, "copy_GBps_read_plus_write": 2 * n / cm / 1e6,
            "replace_passes_GBps_read_plus_write": (n + out_symbols) / max(bm - am, 1e-9) / 1e6}
    print(json.dumps(case), flush=True)
    return case


cases = []
kd, ko = acm.synth.keywords(args.keywords)
m = acm.Machine(1)
m.add_keywords_packed(kd, ko)
n = 1 << args.log2
table = [np.concatenate([kd[ko[k]:ko[k + 1]][::-1], np.array([ord("+")], np.uint8)]) for k in range(args.keywords)]
cases.append(measure("config 2 dictionary, lengths change", m, acm.synth.device_text(n, kd, ko), n, table))
m = acm.Machine(1)
for c in range(97, 123):
    m.add_keyword(bytes([c]))
n = 1 << args.dense_log2
dense = torch.randint(97, 123, (n,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(26))
cases.append(measure("a-z, every symbol a match", m, dense, n, [bytes([c]).upper() * (1 + c % 3) for c in range(97, 123)]))
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_replace.py: ms per call, medians of %d rounds of about %.1f s each, (a), (b) and (c) alternating" % (
            args.rounds, args.window), "device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
        f.write("\n")
