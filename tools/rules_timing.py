"""Measurement driver: what the keyword rules per text (acm_gpu_rules_device, csrc/dev_rules.h) cost
beside the tally they run behind and beside the route a caller had before them, on a buffer resident
on the device that acm_gpu_split_device has cut into lines:
  (1) acm_gpu_tally_batch_device alone         -- the count matrix: the baseline;
  (2) acm_gpu_rules_device                     -- the same tally and the evaluation behind it;
  (3) tally_batch, the matrix copied to the host, the rules evaluated there with numpy (an index by
      keyword and one pass per rule: far better than a loop over the matrix in Python).
The text is the novel (tests/golden/mrs_dalloway.txt), --copies times over.  Two dictionaries:
  config2 -- bench.py's config 2 (1,000 synthetic keywords): none of them occurs in the novel, so the
             matrix is empty and only the always-rules fire -- the floor of what the evaluation costs;
  novel   -- the novel's own 1,000 most frequent words of three letters or more: a matrix with entries.
The rules are generated (--rules, seed 1): AND of two, OR of three, present-and-absent, 2 of 5, a
count of three or more, in turn, and every 64th rule "k absent" (an always-rule), over uniformly
drawn keywords.  (1) and (2) alternate inside one timed loop with device events around `steps` calls,
several rounds, the median; (3) is wall time around whole calls with a synchronise, a few repetitions,
the median.  (2) is checked against (3)'s answer before anything is timed.  Prints one JSON line per dictionary and writes them to --out."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import lib, _check, absent, present, rule

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rules_timing.json"))
ap.add_argument("--copies", type=int, default=16, help="the novel, this many times over")
ap.add_argument("--rules", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed round")
ap.add_argument("--host-repeats", type=int, default=3)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
NO_MAX = binding.ACM_RULE_NO_MAX


def timed(fn, steps):
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


def generated_rules(n_rules, n_keywords, seed=1):
    rng = np.random.default_rng(seed)
    rules = []
    for r in range(n_rules):
        k = rng.integers(0, n_keywords, 5).tolist()
        if r % 64 == 63:                                                   # an always-rule now and then
            rules.append(rule([absent(k[0])]))
            continue
        rules.append((rule([present(k[0]), present(k[1])]), rule([present(k[0]), present(k[1]), present(k[2])], 1),
                      rule([present(k[0]), absent(k[1])]), rule([present(x) for x in k], 2), rule([present(k[0], 3)]))[r % 5])
    return binding.RuleSet(rules)


raw = open(os.path.join(ROOT, "tests", "golden", "mrs_dalloway.txt"), "rb").read()
host_text = np.frombuffer(raw * args.copies, np.uint8)
results = []
for name in ("config2", "novel"):
    m = acm.Machine(1)
    if name == "config2":
        kd, ko = acm.synth.keywords(1000)
        m.add_keywords_packed(kd, ko)
    else:
        seen = {}
        for w in re.findall(rb"[A-Za-z]{3,}", raw):
            seen[w] = seen.get(w, 0) + 1
        for w in sorted(seen, key=lambda w: (-seen[w], w))[:1000]:
            m.add_keyword(w)
    K = m.nb_keywords
    plan = m.plan(0)
    text = torch.from_numpy(host_text.copy()).cuda()
    n = text.numel()
    off = plan.split(text)
    n_texts = off.numel() - 1
    rs = generated_rules(args.rules, K)
    R = plan.rules_create(rs)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    whole = int(plan.count(text, count=cnt).item())
    window = 1 << 24
    capacity = pair_capacity = whole + 4096

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

    # (3) on the host: the matrix indexed by keyword, then every rule in one pass over its terms' entries
    terms_of = [rs.terms[int(rs.rule_ptr[r]):int(rs.rule_ptr[r + 1])].tolist() for r in range(rs.n_rules)]
    base = np.array([sum(1 for t in ts if t[1] == 0) for ts in terms_of], np.int32)

    def host_route():
        tally_batch()
        nnz = int(res[0].item())
        rp, c, v = row_ptr.cpu().numpy(), col[:nnz].cpu().numpy(), val[:nnz].cpu().numpy()
        rows = np.repeat(np.arange(n_texts), np.diff(rp))
        order = np.argsort(c, kind="stable")
        c, rows, v = c[order], rows[order], v[order]
        start = np.searchsorted(c, np.arange(K + 1))
        hits = np.zeros(rs.n_rules, np.int64)
        for r, ts in enumerate(terms_of):
            held = np.full(n_texts, base[r], np.int32)
            for k, lo, hi in ts:
                a, b = start[k], start[k + 1]
                now = (v[a:b] >= lo) & ((v[a:b] <= hi) if hi != NO_MAX else True)
                held[rows[a:b]] += now.astype(np.int32) - (1 if lo == 0 else 0)     # (a keyword occurs once in a row)
            hits[r] = np.count_nonzero(held >= rs.need[r])
        return hits

    # (2)
    want_hits = host_route()
    n_fired = int(want_hits.sum())
    fired_ptr = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
    fired = torch.zeros(max(n_fired, 1), dtype=torch.int32, device="cuda")
    rres = torch.zeros(4, dtype=torch.int64, device="cuda")
    r_bytes = L.acm_gpu_rules_tmp_bytes(plan.h, R.h, window, capacity, pair_capacity, n, n_texts)
    r_tmp = torch.empty(r_bytes, dtype=torch.uint8, device="cuda")

    def rules():
        _check(L.acm_gpu_rules_device(plan.h, R.h, text.data_ptr(), n, off.data_ptr(), n_texts, window, capacity, pair_capacity, fired_ptr.data_ptr(),
                                      fired.data_ptr(), n_fired, rres.data_ptr(), rres.data_ptr() + 8, rres.data_ptr() + 16, rres.data_ptr() + 24,
                                      r_tmp.data_ptr(), r_bytes, st), "acm_gpu_rules_device")

    rules()
    got = [int(x) for x in rres.cpu()]
    assert got[0] == n_fired and got[2] <= capacity and got[3] <= pair_capacity, (got, n_fired)
    assert np.array_equal(np.bincount(fired[:n_fired].cpu().numpy().astype(np.int64), minlength=rs.n_rules), want_hits)
    before = R.info()
    rules()
    after = R.info()
    r, steps = measure({"tally_batch": tally_batch, "rules": rules})
    host = []
    for _ in range(args.host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        host.append((time.perf_counter() - t0) * 1e3)
    plan.status()
    info = R.info()
    out = {"what": "tools/rules_timing.py: ms per call; (1), (2): medians of %d rounds of about %.1f s each, alternating, device events; (3): median "
                   "wall time of %d calls" % (args.rounds, args.window, args.host_repeats),
           "device": torch.cuda.get_device_name(0), "dictionary": name, "keywords": K, "kernel": int(plan.info.kernel), "text_bytes": n, "texts": n_texts,
           "rules": info["rules"], "terms": info["terms"], "postings": info["postings"], "always_rules": info["always_rules"],
           "records": got[1], "matrix_entries": int(res[0].item()), "fired": n_fired,
           "fast_texts_per_call": after["fast_texts"] - before["fast_texts"], "wide_texts_per_call": after["wide_texts"] - before["wide_texts"],
           "steps_per_round": steps, "1_tally_batch_ms": r["tally_batch"][0], "2_rules_ms": r["rules"][0], "3_host_numpy_ms": float(np.median(host)),
           "2_minus_1_over_1": (r["rules"][0] - r["tally_batch"][0]) / r["tally_batch"][0], "rounds_ms": {k: v[1] for k, v in r.items()},
           "host_ms": host}
    print(json.dumps(out), flush=True)
    results.append(out)
    R.close()
    plan.close()
with open(args.out, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("wrote", args.out)
