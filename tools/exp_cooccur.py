"""Measurement driver: what the keyword co-occurrence matrix of a batch (acm_gpu_cooccur_device, csrc/dev_cooccur.h)
costs beside the tally it sits behind (acm_gpu_tally_batch_device, code this feature does not touch), on the batch of
tools/exp_index.py: the novel (tests/golden/mrs_dalloway.txt) --copies times over (4: 1.5 MB), cut into lines by
acm_gpu_split_device, under the novel's own 1,000 most frequent words of three letters or more.
  (1) acm_gpu_tally_batch_device alone                       -- the count matrix whose pairs are counted;
  (2) acm_gpu_cooccur_device, flags 0                        -- (1) and the pair passes behind it;
  (3) acm_gpu_cooccur_matrix_device, flags 0, count only     -- everything but the fill: keys sorted alone;
  (4) the same with room                                     -- and the fill;
  (5) the same under PRODUCT | DIAGONAL                      -- pairs sorted, the weights' running sum;
  (6) acm_gpu_cooccur_add_device of (4)'s matrix with itself -- ADD: 2 nnz entries through the same passes.
The six alternate inside one timed loop with device events around `steps` calls, several rounds, the median.
(2), (5) and (6) are checked against acm_cooccur_matrix / acm_cooccur_add on the host before anything is timed.
Prints one JSON line and writes it to --out."""
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
from aho_corasick_1975_amd.binding import lib, _check

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cooccur.json"))
ap.add_argument("--copies", type=int, default=4, help="the novel, this many times over")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
BOTH = binding.ACM_COOCCUR_PRODUCT | binding.ACM_COOCCUR_DIAGONAL


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


# the expected matrices: the host function on tally_batch's matrix
tally_batch()
torch.cuda.synchronize()
entries = int(res[0].item())
tallied = binding.TalliedBatch(row_ptr.cpu().numpy().view(np.uint64), col[:entries].cpu().numpy().view(np.uint32),
                               val[:entries].cpu().numpy().view(np.uint64), entries, 0)
want = {flags: binding.cooccur_matrix(tallied, flags, 0, K) for flags in (0, BOTH)}
cross = max(w.cross for w in want.values())
room = max(w.nnz for w in want.values())
co_ptr = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
co_col = torch.zeros(2 * room, dtype=torch.int32, device="cuda")
co_val = torch.zeros(2 * room, dtype=torch.int64, device="cuda")
cres = torch.zeros(6, dtype=torch.int64, device="cuda")                    # nnz, total, need, need_pairs, cross, skipped
c_bytes = L.acm_gpu_cooccur_tmp_bytes(plan.h, window, capacity, pair_capacity, n, n_texts, K, cross)
m_bytes = L.acm_gpu_cooccur_matrix_tmp_bytes(plan.h, n_texts, K, cross)
c_tmp = torch.empty(c_bytes, dtype=torch.uint8, device="cuda")
m_tmp = torch.empty(m_bytes, dtype=torch.uint8, device="cuda")
r = cres.data_ptr()


def cooccur(flags=0):
    _check(L.acm_gpu_cooccur_device(plan.h, text.data_ptr(), n, off.data_ptr(), n_texts, window, capacity, pair_capacity, K, flags, 0, cross,
                                    co_ptr.data_ptr(), co_col.data_ptr(), co_val.data_ptr(), room, r, r + 32, r + 40, r + 8, r + 16, r + 24,
                                    c_tmp.data_ptr(), c_bytes, st), "acm_gpu_cooccur_device")


def matrix(flags=0, fill=True):
    _check(L.acm_gpu_cooccur_matrix_device(plan.h, row_ptr.data_ptr(), col.data_ptr(), val.data_ptr(), n_texts, K, flags, 0, cross, co_ptr.data_ptr(),
                                           co_col.data_ptr() if fill else None, co_val.data_ptr() if fill else None, room if fill else 0, r, r + 32, r + 40,
                                           m_tmp.data_ptr(), m_bytes, st), "acm_gpu_cooccur_matrix_device")


def same(w):
    return (np.array_equal(co_ptr.cpu().numpy().view(np.uint64), w.co_ptr) and np.array_equal(co_col.cpu().numpy().view(np.uint32)[:w.nnz], w.co_col) and
            np.array_equal(co_val.cpu().numpy().view(np.uint64)[:w.nnz], w.co_val))


cooccur()
got = [int(x) for x in cres.cpu()]
assert got[0] == want[0].nnz and got[2] <= capacity and got[3] <= pair_capacity and got[4] == want[0].cross and same(want[0]), got
matrix(BOTH)
assert same(want[BOTH]) and int(cres[4].item()) == want[BOTH].cross
# ADD: the matrix of flags 0 with itself
matrix(0)
a_ptr, a_col, a_val = co_ptr.clone(), co_col[:want[0].nnz].clone(), co_val[:want[0].nnz].clone()
a_bytes = L.acm_gpu_cooccur_add_tmp_bytes(plan.h, K, 2 * want[0].nnz)
a_tmp = torch.empty(a_bytes, dtype=torch.uint8, device="cuda")


def add():
    _check(L.acm_gpu_cooccur_add_device(plan.h, a_ptr.data_ptr(), a_col.data_ptr(), a_val.data_ptr(), K, a_ptr.data_ptr(), a_col.data_ptr(),
                                        a_val.data_ptr(), K, 2 * want[0].nnz, co_ptr.data_ptr(), co_col.data_ptr(), co_val.data_ptr(), 2 * room, r, r + 32,
                                        a_tmp.data_ptr(), a_bytes, st), "acm_gpu_cooccur_add_device")


add()
assert same(binding.cooccur_add(want[0], want[0]))
t, steps = measure({"tally_batch": tally_batch, "cooccur": cooccur, "count_only": lambda: matrix(0, False), "matrix": matrix,
                    "matrix_product_diagonal": lambda: matrix(BOTH), "add": add})
plan.status()
tb, co, c0, mx, pd, ad = (t[x][0] for x in ("tally_batch", "cooccur", "count_only", "matrix", "matrix_product_diagonal", "add"))
row_len = np.diff(tallied.row_ptr.astype(np.int64))
out = {"what": "tools/exp_cooccur.py: ms per call; medians of %d rounds of about %.1f s each, the six calls alternating, device events" % (
           args.rounds, args.window),
       "device": torch.cuda.get_device_name(0), "keywords": K, "kernel": int(plan.info.kernel), "text_bytes": n, "texts": n_texts, "records": got[1],
       "matrix_entries": entries, "widest_row": int(row_len.max()), "median_row": int(np.median(row_len)),
       "pair_instances": {"plain": want[0].cross, "diagonal": want[BOTH].cross}, "nnz": {"plain": want[0].nnz, "diagonal": want[BOTH].nnz},
       "greatest_value": int(want[0].co_val.max()), "scratch_bytes_matrix": m_bytes, "steps_per_round": steps,
       "1_tally_batch_ms": tb, "2_cooccur_ms": co, "3_matrix_count_only_ms": c0, "4_matrix_ms": mx, "5_matrix_product_diagonal_ms": pd, "6_add_ms": ad,
       "cooccur_over_tally": co / tb, "pair_passes_in_the_call_ms": co - tb, "fill_passes_ms": mx - c0, "weights_cost_ms": pd - mx,
       "pair_instances_per_second": want[0].cross / (mx * 1e-3), "rounds_ms": {k: v[1] for k, v in t.items()}}
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump([out], f, indent=1)
    f.write("\n")
print("wrote", args.out)
