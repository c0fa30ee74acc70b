"""Experiment driver: what the whole-word filter costs beside the ordered scan it runs behind.
acm_gpu_scan_words_device is acm_gpu_scan_ordered_device (emit_from = 0) into scratch plus the two
passes of csrc/dev_words.h over the records.  This times, in one process and on one build, on config
2's workload (the 1,000-keyword synthetic dictionary, 1 GiB of a-z text resident on the device),
  (a) acm_gpu_scan_ordered_device of the buffer (this change does not touch it: the figure is the
      parent commit's);
  (b) acm_gpu_scan_words_device of the same buffer into the same record room;
  (c) acm_gpu_words_records_device alone on the records (a) left, count read on the device;
  (d) the same on --records hand-made records in position order (one per 64 symbols, length 4): the
      filter at a size where launches no longer dominate, in records per second.
The text holds letters only, so the word set is a-m: a neighbour is a word symbol or not by its
letter, about a quarter of the records pass ACM_WORDS_BOTH.  (a) .. (d) alternate inside one timed
loop, several rounds, every round ending in a device synchronise; ms per call, medians.  (c)'s and
(d)'s outputs are checked against numpy's evaluation of the definition before anything is timed.
The expectation from the passes: (b) = (a) + (c) + the time the scan's records take to be written to
scratch and read from there instead of the caller's array (none: same bytes).  Prints one JSON line
and writes it to --out if given."""
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
from aho_corasick_1975_amd.binding import lib, _check, RECORD_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--log2", type=int, default=30)
ap.add_argument("--keywords", type=int, default=1000)
ap.add_argument("--records", type=int, default=1 << 24)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
n = 1 << args.log2
RANGES = np.array([ord("a"), ord("m")], np.uint8)


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def by_definition(text, rec):
    """ACM_WORDS_BOTH over one text, word set a-m, with numpy: the kept records in input order"""
    end = rec["end_pos"].astype(np.int64)
    start = end + 1 - rec["length"].astype(np.int64)
    left = text[np.maximum(start - 1, 0)]
    right = text[np.minimum(end + 1, text.size - 1)]
    left_ok = (start == 0) | (left < ord("a")) | (left > ord("m"))
    right_ok = (end + 1 == text.size) | (right < ord("a")) | (right > ord("m"))
    return rec[left_ok & right_ok]


kd, ko = acm.synth.keywords(args.keywords)
m = acm.Machine(1)
m.add_keywords_packed(kd, ko)
plan = m.plan(0)
text = acm.synth.device_text(n, kd, ko)
host_text = text.cpu().numpy()
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
cnt_out = torch.zeros(1, dtype=torch.int64, device="cuda")
cap = int(plan.count(text).item()) + 4096
rec = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
kept = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
to = L.acm_gpu_scan_ordered_tmp_bytes(plan.h, cap, n)
tw = L.acm_gpu_scan_words_tmp_bytes(plan.h, cap, n, 0)
tf = L.acm_gpu_words_tmp_bytes(plan.h, cap, 0)
tmp = torch.empty(max(to, tw, tf), dtype=torch.uint8, device="cuda")

# (d)'s records: one per 64 symbols, length 4, position order
n_big = min(args.records, n // 64 - 1)
big = np.zeros(n_big, RECORD_DTYPE)
big["end_pos"] = np.arange(n_big, dtype=np.uint64) * np.uint64(64) + np.uint64(35)
big["length"] = 4
d_big = torch.from_numpy(big.view(np.int64).reshape(-1, 2).copy()).cuda()
d_big_out = torch.empty_like(d_big)
tb = L.acm_gpu_words_tmp_bytes(plan.h, n_big, 0)
tmp_big = torch.empty(tb, dtype=torch.uint8, device="cuda")


def ordered():
    _check(L.acm_gpu_scan_ordered_device(plan.h, text.data_ptr(), n, 0, 0, rec.data_ptr(), cap, cnt.data_ptr(), tmp.data_ptr(), to, st),
           "acm_gpu_scan_ordered_device")


def scan_words():
    _check(L.acm_gpu_scan_words_device(plan.h, text.data_ptr(), n, 0, None, 0, RANGES.ctypes.data, 1, 3, kept.data_ptr(), cap, cnt_out.data_ptr(),
                                       tmp.data_ptr(), tw, st), "acm_gpu_scan_words_device")


def words_alone():
    _check(L.acm_gpu_words_records_device(plan.h, text.data_ptr(), n, 0, None, 0, RANGES.ctypes.data, 1, 3, rec.data_ptr(), cap, cnt.data_ptr(),
                                          kept.data_ptr(), cnt_out.data_ptr(), tmp.data_ptr(), tf, st), "acm_gpu_words_records_device")


def words_big():
    _check(L.acm_gpu_words_records_device(plan.h, text.data_ptr(), n, 0, None, 0, RANGES.ctypes.data, 1, 3, d_big.data_ptr(), n_big, None,
                                          d_big_out.data_ptr(), cnt_out.data_ptr(), tmp_big.data_ptr(), tb, st), "acm_gpu_words_records_device")


def host_records(t, k):
    return np.frombuffer(t[:k].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)


ordered()
torch.cuda.synchronize()
records_in = int(cnt.item())
want = by_definition(host_text, host_records(rec, records_in))
words_alone()
torch.cuda.synchronize()
records_out = int(cnt_out.item())
assert records_out == want.size and np.array_equal(host_records(kept, records_out), want), (records_out, want.size)
scan_words()
torch.cuda.synchronize()
assert int(cnt_out.item()) == want.size and np.array_equal(host_records(kept, want.size), want)
words_big()
torch.cuda.synchronize()
big_out = int(cnt_out.item())
want_big = by_definition(host_text, big)
assert big_out == want_big.size and np.array_equal(host_records(d_big_out, big_out), want_big), (big_out, want_big.size)
assert 0 < records_out < records_in <= cap and 0 < big_out < n_big
plan.status()
fns = {"a_scan_ordered": ordered, "b_scan_words": scan_words, "c_words_records": words_alone, "d_words_records_big": words_big}
for fn in list(fns.values()) * 2:                                 # warm-up of every shape
    fn()
steps = max(5, int(args.window * 1e3 / max(timed(scan_words, 5), 1e-3)))
rounds = {k: [] for k in fns}
for _ in range(args.rounds):                                      # alternating, so that drift hits all alike
    for k, fn in fns.items():
        rounds[k].append(timed(fn, steps))
med = {k: float(np.median(v)) for k, v in rounds.items()}
case = {"keywords": args.keywords, "text_bytes": n, "kernel": int(plan.info.kernel), "word_set": "a-m", "flags": "both",
        "records_in": records_in, "records_out": records_out, "big_records_in": n_big, "big_records_out": big_out, "steps_per_round": steps,
        "tmp_bytes_ordered": int(to), "tmp_bytes_scan_words": int(tw), "tmp_bytes_words": int(tf), "tmp_bytes_words_big": int(tb),
        "ms": med, "rounds_ms": rounds,
        "b_minus_a_ms": med["b_scan_words"] - med["a_scan_ordered"], "b_over_a": med["b_scan_words"] / med["a_scan_ordered"],
        "c_records_per_s": records_in / (med["c_words_records"] * 1e-3), "d_records_per_s": n_big / (med["d_words_records_big"] * 1e-3),
        "d_bytes_per_record": 16 + 2 + 2 * 8 / 64 + 32 * big_out / n_big}
print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_words.py: ms per call, medians of %d rounds of about %.1f s each, (a) .. (d) alternating" % (
            args.rounds, args.window), "device": torch.cuda.get_device_name(0), "case": case}, f, indent=1)
        f.write("\n")
