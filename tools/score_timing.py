"""Measurement driver: what the weighted scores per text (acm_gpu_score_device, csrc/dev_score.h) cost beside
the keyword rules (acm_gpu_rules_device, csrc/dev_rules.h) on the batch of tools/rules_timing.py: the novel
(tests/golden/mrs_dalloway.txt) --copies times over, cut into lines by acm_gpu_split_device, under the novel's
own 1,000 most frequent words of three letters or more.
  (1) acm_gpu_tally_batch_device alone          -- the count matrix both run behind;
  (2) acm_gpu_rules_device                      -- rules_timing.py's generated rule set;
  (3) acm_gpu_score_device, k = 0               -- a model with one class per rule and one term per rule term,
                                                   so the same number of postings on the same keywords;
  (4) acm_gpu_score_device, k = 10              -- the same with the top pass.
The four alternate inside one timed loop with device events around `steps` calls, several rounds, the median.
(3) is checked against acm_score_matrix and acm_score_top on the host before anything is timed.  Prints one
JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import lib, _check, absent, present, rule, score_class, weight

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.json"))
ap.add_argument("--copies", type=int, default=16, help="the novel, this many times over")
ap.add_argument("--rules", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed round")
ap.add_argument("--k", type=int, default=10)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()


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


def generated(n_rules, n_keywords, seed=1):
    """rules_timing.py's rule set, and the model that has a term (same keyword) for every term of it: a weight of 1 to 9
    where the rule wants the keyword present, -1 to -9 where it wants it absent, a cap where the rule counts"""
    rng = np.random.default_rng(seed)
    wrng = np.random.default_rng(seed + 1)
    rules, classes = [], []
    for r in range(n_rules):
        k = rng.integers(0, n_keywords, 5).tolist()
        w = wrng.integers(1, 10, 5).tolist()
        if r % 64 == 63:                                                   # an always-rule, an always-class now and then
            rules.append(rule([absent(k[0])]))
            classes.append(score_class([weight(k[0], -w[0])], bias=1, threshold=1))
            continue
        rules.append((rule([present(k[0]), present(k[1])]), rule([present(k[0]), present(k[1]), present(k[2])], 1),
                      rule([present(k[0]), absent(k[1])]), rule([present(x) for x in k], 2), rule([present(k[0], 3)]))[r % 5])
        classes.append((score_class([weight(k[0], w[0]), weight(k[1], w[1])], threshold=w[0] + w[1]),
                        score_class([weight(k[0], w[0]), weight(k[1], w[1]), weight(k[2], w[2])]),
                        score_class([weight(k[0], w[0], 1), weight(k[1], -w[1])]),
                        score_class([weight(x, y, 1) for x, y in zip(k, w)], threshold=min(w) + 1),
                        score_class([weight(k[0], w[0], 3)], threshold=3 * w[0]))[r % 5])
    return binding.RuleSet(rules), binding.ScoreModel(classes)


raw = open(os.path.join(ROOT, "tests", "golden", "mrs_dalloway.txt"), "rb").read()
host_text = np.frombuffer(raw * args.copies, np.uint8)
m = acm.Machine(1)
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
rs, sm = generated(args.rules, K)
R, S = plan.rules_create(rs), plan.score_create(sm)
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
                                        col.data_ptr(), val.data_ptr(), res.data_ptr(), res.data_ptr() + 8, res.data_ptr() + 16, res.data_ptr() + 24,
                                        tb_tmp.data_ptr(), tb_bytes, st), "acm_gpu_tally_batch_device")


n_fired = plan.rules(text, off, R, window=window, capacity=capacity, pair_capacity=pair_capacity, fired_capacity=0).n_fired
fired_ptr = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
fired = torch.zeros(max(n_fired, 1), dtype=torch.int32, device="cuda")
rres = torch.zeros(4, dtype=torch.int64, device="cuda")
r_bytes = L.acm_gpu_rules_tmp_bytes(plan.h, R.h, window, capacity, pair_capacity, n, n_texts)
r_tmp = torch.empty(r_bytes, dtype=torch.uint8, device="cuda")


def rules():
    _check(L.acm_gpu_rules_device(plan.h, R.h, text.data_ptr(), n, off.data_ptr(), n_texts, window, capacity, pair_capacity, fired_ptr.data_ptr(),
                                  fired.data_ptr(), n_fired, rres.data_ptr(), rres.data_ptr() + 8, rres.data_ptr() + 16, rres.data_ptr() + 24,
                                  r_tmp.data_ptr(), r_bytes, st), "acm_gpu_rules_device")


# the expected result of (3) and (4): the host functions on tally_batch's matrix
tally_batch()
torch.cuda.synchronize()
nnz = int(res[0].item())
tallied = binding.TalliedBatch(row_ptr.cpu().numpy().view(np.uint64), col[:nnz].cpu().numpy().view(np.uint32), val[:nnz].cpu().numpy().view(np.uint64), nnz, 0)
want = binding.score_top(binding.score_matrix(tallied, sm, K), sm.n_classes, args.k)
n_kept = want.n_kept
kept_ptr = torch.zeros(n_texts + 1, dtype=torch.int64, device="cuda")
kept_class = torch.zeros(max(n_kept, 1), dtype=torch.int32, device="cuda")
kept_score = torch.zeros(max(n_kept, 1), dtype=torch.int64, device="cuda")
best = torch.zeros(n_texts, dtype=torch.int32, device="cuda")
hits = torch.zeros(sm.n_classes, dtype=torch.int64, device="cuda")
top_n = torch.zeros(sm.n_classes, dtype=torch.int32, device="cuda")
top_text = torch.zeros(sm.n_classes * args.k, dtype=torch.int32, device="cuda")
top_score = torch.zeros(sm.n_classes * args.k, dtype=torch.int64, device="cuda")
sres = torch.zeros(4, dtype=torch.int64, device="cuda")
s_tmp = {}
for k in (0, args.k):
    b = L.acm_gpu_score_tmp_bytes(plan.h, S.h, window, capacity, pair_capacity, n, n_texts, n_kept, k)
    s_tmp[k] = (torch.empty(b, dtype=torch.uint8, device="cuda"), b)


def score(k):
    tmp, b = s_tmp[k]
    _check(L.acm_gpu_score_device(plan.h, S.h, text.data_ptr(), n, off.data_ptr(), n_texts, window, capacity, pair_capacity, kept_ptr.data_ptr(),
                                  kept_class.data_ptr(), kept_score.data_ptr(), n_kept, sres.data_ptr(), best.data_ptr(), k, hits.data_ptr(),
                                  top_n.data_ptr(), top_text.data_ptr(), top_score.data_ptr(), sres.data_ptr() + 8, sres.data_ptr() + 16,
                                  sres.data_ptr() + 24, tmp.data_ptr(), b, st), "acm_gpu_score_device")


score(args.k)
got = [int(x) for x in sres.cpu()]
assert got[0] == n_kept and got[2] <= capacity and got[3] <= pair_capacity, (got, n_kept)
assert np.array_equal(kept_ptr.cpu().numpy().view(np.uint64), want.kept_ptr) and np.array_equal(kept_class.cpu().numpy().view(np.uint32)[:n_kept], want.kept_class)
assert np.array_equal(kept_score.cpu().numpy()[:n_kept], want.kept_score) and np.array_equal(best.cpu().numpy().view(np.uint32), want.best)
assert np.array_equal(hits.cpu().numpy().view(np.uint64), want.class_hits) and np.array_equal(top_text.cpu().numpy().view(np.uint32), want.top_text.reshape(-1))
assert np.array_equal(top_score.cpu().numpy(), want.top_score.reshape(-1))
before = S.info()
score(0)
after = S.info()
r, steps = measure({"tally_batch": tally_batch, "rules": rules, "score_k0": lambda: score(0), "score_top": lambda: score(args.k)})
plan.status()
ri, si = R.info(), S.info()
t, ru, s0, sk = (r[x][0] for x in ("tally_batch", "rules", "score_k0", "score_top"))
out = {"what": "tools/score_timing.py: ms per call; medians of %d rounds of about %.1f s each, the four calls alternating, device events" % (
           args.rounds, args.window),
       "device": torch.cuda.get_device_name(0), "keywords": K, "kernel": int(plan.info.kernel), "text_bytes": n, "texts": n_texts,
       "records": got[1], "matrix_entries": nnz,
       "rules": ri["rules"], "rule_terms": ri["terms"], "rule_postings": ri["postings"], "always_rules": ri["always_rules"], "fired": n_fired,
       "classes": si["classes"], "score_terms": si["terms"], "score_postings": si["postings"], "always_classes": si["always_classes"], "kept": n_kept,
       "k": args.k, "longest_column": int(want.class_hits.max()),
       "fast_texts_per_call": after["fast_texts"] - before["fast_texts"], "wide_texts_per_call": after["wide_texts"] - before["wide_texts"],
       "steps_per_round": steps, "1_tally_batch_ms": t, "2_rules_ms": ru, "3_score_k0_ms": s0, "4_score_top_ms": sk,
       "rules_pass_ms": ru - t, "score_pass_ms": s0 - t, "score_pass_over_rules_pass": (s0 - t) / (ru - t), "top_pass_ms": sk - s0,
       "rounds_ms": {k: v[1] for k, v in r.items()}}
print(json.dumps(out), flush=True)
with open(args.out, "w") as f:
    json.dump([out], f, indent=1)
    f.write("\n")
print("wrote", args.out)
