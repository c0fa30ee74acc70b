"""Measurement driver: what the inverted index of a batch (acm_gpu_index_device, csrc/dev_index.h) costs beside the
tally it sits behind (acm_gpu_tally_batch_device, code this feature does not touch), on the batch of
tools/score_timing.py: the novel (tests/golden/mrs_dalloway.txt) --copies times over (16: 5.9 MB), cut into lines by
acm_gpu_split_device, under the novel's own 1,000 most frequent words of three letters or more.  The dictionary is
skewed as word counts are: `the` and `and` are in every other line, the 1,000th word in a handful.
  (1) acm_gpu_tally_batch_device alone                   -- the count matrix the index is the transposition of;
  (2) acm_gpu_index_device                               -- (1) and the transposition behind it;
  (3) acm_gpu_index_matrix_device, count only            -- passes 1 to 3: the check, the counts, post_ptr (df);
  (4) the same with room, ACM_GPU_INDEX_LIST absent      -- 1,024: the short lists in LDS, the long ones by the radix sort;
  (5) the same, ACM_GPU_INDEX_LIST = 4096                -- the fast form takes what it can;
  (6) the same, ACM_GPU_INDEX_LIST = 1                   -- every list of two or more by the wide form.
The six alternate inside one timed loop with device events around `steps` calls, several rounds, the median.
(2) is checked against acm_index_matrix on the host before anything is timed.  Prints one JSON line and writes it
to --out."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index.json"))
ap.add_argument("--copies", type=int, default=16, help="the novel, this many times over")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
ENV = "ACM_GPU_INDEX_LIST"


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


def with_list(value, fn):
    """fn () with ACM_GPU_INDEX_LIST = value (None: absent); the library reads it at every call"""
    def run():
        if value is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = str(value)
        fn()
        os.environ.pop(ENV, None)
    return run


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


# the expected index: the host function on tally_batch's matrix
tally_batch()
torch.cuda.synchronize()
nnz = int(res[0].item())
tallied = binding.TalliedBatch(row_ptr.cpu().numpy().view(np.uint64), col[:nnz].cpu().numpy().view(np.uint32), val[:nnz].cpu().numpy().view(np.uint64), nnz, 0)
want = binding.index_matrix(tallied, K)
df = np.diff(want.post_ptr.astype(np.int64))
post_ptr = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
post_text = torch.zeros(max(nnz, 1), dtype=torch.int32, device="cuda")
post_count = torch.zeros(max(nnz, 1), dtype=torch.int64, device="cuda")
ires = torch.zeros(6, dtype=torch.int64, device="cuda")                    # nnz, total, need, need_pairs, forms[2]
os.environ[ENV] = "1"                                                      # (the largest scratch: a sort room whatever the list)
i_bytes = L.acm_gpu_index_tmp_bytes(plan.h, window, capacity, pair_capacity, n, n_texts, K, nnz)
m_bytes = L.acm_gpu_index_matrix_tmp_bytes(plan.h, n_texts, K, nnz)
os.environ.pop(ENV)
i_tmp = torch.empty(i_bytes, dtype=torch.uint8, device="cuda")
m_tmp = torch.empty(m_bytes, dtype=torch.uint8, device="cuda")


def index():
    _check(L.acm_gpu_index_device(plan.h, text.data_ptr(), n, off.data_ptr(), n_texts, window, capacity, pair_capacity, K, 0, post_ptr.data_ptr(),
                                  post_text.data_ptr(), post_count.data_ptr(), nnz, ires.data_ptr(), ires.data_ptr() + 32, ires.data_ptr() + 8,
                                  ires.data_ptr() + 16, ires.data_ptr() + 24, i_tmp.data_ptr(), i_bytes, st), "acm_gpu_index_device")


def transpose(fill=True):
    _check(L.acm_gpu_index_matrix_device(plan.h, row_ptr.data_ptr(), col.data_ptr(), val.data_ptr(), n_texts, K, 0, post_ptr.data_ptr(),
                                         post_text.data_ptr() if fill else None, post_count.data_ptr() if fill else None, nnz if fill else 0,
                                         ires.data_ptr(), ires.data_ptr() + 32, m_tmp.data_ptr(), m_bytes, st), "acm_gpu_index_matrix_device")


def same():
    return (np.array_equal(post_ptr.cpu().numpy().view(np.uint64), want.post_ptr) and
            np.array_equal(post_text.cpu().numpy().view(np.uint32)[:nnz], want.post_text) and
            np.array_equal(post_count.cpu().numpy().view(np.uint64)[:nnz], want.post_count))


index()
got = [int(x) for x in ires.cpu()]
assert got[0] == nnz and got[2] <= capacity and got[3] <= pair_capacity and same(), got
forms = {}
for value in (None, 4096, 1):
    post_text.zero_()
    with_list(value, transpose)()
    forms[value] = [int(x) for x in ires.cpu()][4:]
    assert same(), value
r, steps = measure({"tally_batch": tally_batch, "index": index, "count_only": lambda: transpose(False), "list_default": with_list(None, transpose),
                    "list_4096": with_list(4096, transpose), "list_1": with_list(1, transpose)})
plan.status()
t, ix, c0, d, big, one = (r[x][0] for x in ("tally_batch", "index", "count_only", "list_default", "list_4096", "list_1"))
out = {"what": "tools/exp_index.py: ms per call; medians of %d rounds of about %.1f s each, the six calls alternating, device events" % (
           args.rounds, args.window),
       "device": torch.cuda.get_device_name(0), "keywords": K, "kernel": int(plan.info.kernel), "text_bytes": n, "texts": n_texts,
       "records": got[1], "matrix_entries": nnz, "longest_list": int(df.max()), "median_list": int(np.median(df)), "empty_lists": int(np.count_nonzero(df == 0)),
       "lists_over_256": int(np.count_nonzero(df > 256)), "lists_over_1024": int(np.count_nonzero(df > 1024)), "lists_over_4096": int(np.count_nonzero(df > 4096)),
       "forms_fast_wide": {str(k): v for k, v in forms.items()}, "steps_per_round": steps,
       "1_tally_batch_ms": t, "2_index_ms": ix, "3_transpose_count_only_ms": c0, "4_transpose_list_1024_ms": d, "5_transpose_list_4096_ms": big,
       "6_transpose_list_1_ms": one, "index_over_tally": ix / t, "transposition_in_the_call_ms": ix - t, "fill_passes_ms": d - c0,
       "rounds_ms": {k: v[1] for k, v in r.items()}}
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump([out], f, indent=1)
    f.write("\n")
print("wrote", args.out)
