"""Experiment driver: what the anchored walk costs beside the batch scan a caller had to run before it.
Until acm_gpu_lookup_device, "is this cell a keyword" and "which keyword does this line begin with" were
acm_gpu_scan_batch_device and a filter on the host: all matches of the concatenation found, ordered and
cut per text, nearly all of them thrown away.  This times, in one process and on one build, alternating,
  (a) acm_gpu_scan_batch_device on the batch (this change does not touch it: the parent's route);
  (b) acm_gpu_lookup_device, all three arrays;
  (c) acm_gpu_scan_anchored_device, ACM_ANCHORED_PREFIXES, capacity = n_texts;
on two workloads of at least --mib MiB of a-z text each, under two dictionaries (--keywords: the 1,000
keywords of config 2, a dense plan; 20,000 keywords, a 4-gram plan):
  cells: texts of a mean of 8 symbols, one in four a keyword and nothing else (set membership, a column's
         dictionary encoding);
  lines: texts of a mean of 80 symbols, one in four beginning with a keyword (a verb, a tag).
Every round gives each figure at least --window seconds of work, timed between two device events;
ms per call, the median of the rounds and their spread (max - min over the median).  Beside them:
texts per second, and the bytes of text the walk can read at most -- sum over t of min (len_t, lmax),
counted on the host from the offsets -- over the time.  Before anything is timed (c)'s records are
compared with (a)'s filtered by the definition in numpy, and (b)'s arrays with what follows from
them.  Prints one JSON line per case and writes all to --out if given."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.binding import lib, _check, RECORD_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--mib", type=int, default=128)
ap.add_argument("--keywords", type=int, nargs="*", default=[1000, 20000])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window", type=float, default=1.0, help="seconds of work per figure and round")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measures the GPU: no device, no numbers"
torch.cuda.set_device(0)
L = lib()
NONE = 0xFFFFFFFF


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


def make_batch(n, mean, whole, kd, ko, seed):
    """(text, offsets, which texts hold a keyword, which keyword) of at least n symbols of a-z: a text in four
    is a keyword (whole) or begins with one, the rest of every text is random letters, 0 .. 2 * mean of them"""
    rng = np.random.default_rng(seed)
    klen = np.diff(ko).astype(np.int64)
    count = int(n // mean * 1.2) + 16
    is_kw = rng.random(count) < 0.25
    kw = rng.integers(0, klen.size, count)
    tail = rng.integers(0, 2 * mean + 1, count)
    length = np.where(is_kw, klen[kw] + (0 if whole else 1) * tail, tail)
    off = np.zeros(count + 1, np.int64)
    np.cumsum(length, out=off[1:])
    count = int(np.searchsorted(off, n)) + 1                 # the texts up to the first offset at or behind n
    assert count < off.size
    off, is_kw, kw = off[:count + 1], is_kw[:count], kw[:count]
    text = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
    at, which = off[:-1][is_kw], kw[is_kw]
    lens = klen[which]
    local = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    text[np.repeat(at, lens) + local] = kd[np.repeat(ko[which].astype(np.int64), lens) + local]
    return text, off, is_kw, kw


def run_case(n_keywords, name, mean, whole):
    kd, ko = acm.synth.keywords(n_keywords)
    m = acm.Machine(1)
    m.add_keywords_packed(kd, ko)
    plan = m.plan(0)
    lmax = int(np.diff(ko).max())
    text, off, is_kw, kw = make_batch(args.mib << 20, mean, whole, np.asarray(kd), np.asarray(ko), 1975 + mean)
    n, n_texts = text.size, off.size - 1
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cap_a = int(plan.count(d_text).item()) + 4096            # (a) needs room for the matches of the concatenation
    rec_a = torch.empty((cap_a, 2), dtype=torch.int64, device="cuda")
    tid_a = torch.empty(cap_a, dtype=torch.int32, device="cuda")
    first_a = torch.empty(n_texts + 1, dtype=torch.int64, device="cuda")
    cnt_a = torch.zeros(1, dtype=torch.int64, device="cuda")
    ta = L.acm_gpu_scan_batch_tmp_bytes(plan.h, cap_a, n, n_texts)
    tmp_a = torch.empty(ta, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(n_texts, dtype=torch.int32, device="cuda") for _ in range(3)]
    tb = L.acm_gpu_lookup_tmp_bytes(plan.h, n_texts)
    tmp_b = torch.empty(tb, dtype=torch.uint8, device="cuda")
    cap_c = n_texts
    rec_c = torch.empty((cap_c, 2), dtype=torch.int64, device="cuda")
    tid_c = torch.empty(cap_c, dtype=torch.int32, device="cuda")
    first_c = torch.empty(n_texts + 1, dtype=torch.int64, device="cuda")
    cnt_c = torch.zeros(1, dtype=torch.int64, device="cuda")
    tc = L.acm_gpu_scan_anchored_tmp_bytes(plan.h, n_texts)
    tmp_c = torch.empty(tc, dtype=torch.uint8, device="cuda")

    def batch():
        _check(L.acm_gpu_scan_batch_device(plan.h, d_text.data_ptr(), n, d_off.data_ptr(), n_texts, rec_a.data_ptr(), tid_a.data_ptr(), first_a.data_ptr(),
                                           cap_a, cnt_a.data_ptr(), tmp_a.data_ptr(), ta, st), "acm_gpu_scan_batch_device")

    def lookup():
        _check(L.acm_gpu_lookup_device(plan.h, d_text.data_ptr(), n, d_off.data_ptr(), n_texts, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                       tmp_b.data_ptr(), tb, st), "acm_gpu_lookup_device")

    def prefixes():
        _check(L.acm_gpu_scan_anchored_device(plan.h, d_text.data_ptr(), n, d_off.data_ptr(), n_texts, 1, rec_c.data_ptr(), tid_c.data_ptr(),
                                              first_c.data_ptr(), cap_c, cnt_c.data_ptr(), tmp_c.data_ptr(), tc, st), "acm_gpu_scan_anchored_device")

    # ---- the three agree before anything is timed
    batch(), lookup(), prefixes()
    torch.cuda.synchronize()
    n_a, n_c = int(cnt_a.item()), int(cnt_c.item())
    assert n_a <= cap_a and n_c <= cap_c, (n_a, cap_a, n_c, cap_c)
    a = np.frombuffer(rec_a[:n_a].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
    ta_ids = tid_a[:n_a].cpu().numpy().view(np.uint32).astype(np.int64)
    anchored = a["end_pos"].astype(np.int64) + 1 - a["length"].astype(np.int64) == off[ta_ids]
    c = np.frombuffer(rec_c[:n_c].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
    tc_ids = tid_c[:n_c].cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(a[anchored], c) and np.array_equal(ta_ids[anchored], tc_ids), "PREFIXES is the batch scan's anchored records"
    whole_id, prefix_id, prefix_len = [o.cpu().numpy().view(np.uint32) for o in outs]
    last = np.ones(n_c, bool)
    last[:-1] = tc_ids[1:] != tc_ids[:-1]
    want_id, want_len = np.full(n_texts, NONE, np.uint32), np.zeros(n_texts, np.uint32)
    want_id[tc_ids[last]], want_len[tc_ids[last]] = c["keyword_id"][last], c["length"][last]
    assert np.array_equal(prefix_id, want_id) and np.array_equal(prefix_len, want_len)
    assert np.array_equal(whole_id != NONE, (prefix_len == np.diff(off)) & (prefix_len > 0))
    assert np.all(prefix_len[is_kw] >= np.diff(ko)[kw[is_kw]]) and (not whole or np.all(whole_id[is_kw] != NONE))
    plan.status()

    fns = {"a_scan_batch": batch, "b_lookup": lookup, "c_scan_anchored_prefixes": prefixes}
    for fn in list(fns.values()) * 2:                             # warm-up of every shape
        fn()
    steps = {k: max(3, int(np.ceil(args.window * 1e3 / max(timed(fn, 3), 1e-3)))) for k, fn in fns.items()}
    rounds = {k: [] for k in fns}
    for _ in range(args.rounds):                                  # alternating, so that drift hits all alike
        for k, fn in fns.items():
            rounds[k].append(timed(fn, steps[k]))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
    walk_bytes = int(np.minimum(np.diff(off), lmax).sum())
    case = {"workload": name, "keywords": n_keywords, "kernel": int(plan.info.kernel), "lmax": lmax, "text_bytes": int(n), "n_texts": int(n_texts),
            "mean_text": float(n) / n_texts, "batch_records": n_a, "batch_capacity": cap_a, "anchored_records": n_c,
            "texts_with_a_prefix": int(np.count_nonzero(prefix_len)), "texts_whole": int(np.count_nonzero(whole_id != NONE)),
            "tmp_bytes": {"a_scan_batch": int(ta), "b_lookup": int(tb), "c_scan_anchored_prefixes": int(tc)},
            "steps_per_round": steps, "ms": med, "spread": spread, "rounds_ms": rounds,
            "texts_per_s": {k: n_texts / (v * 1e-3) for k, v in med.items()},
            "walk_bytes_at_most": walk_bytes, "walk_bytes_per_s": {k: walk_bytes / (med[k] * 1e-3) for k in ("b_lookup", "c_scan_anchored_prefixes")},
            "a_over_b": med["a_scan_batch"] / med["b_lookup"], "a_over_c": med["a_scan_batch"] / med["c_scan_anchored_prefixes"]}
    print(json.dumps(case), flush=True)
    return case


cases = []
for nk in args.keywords:
    cases.append(run_case(nk, "cells", 8, True))
    cases.append(run_case(nk, "lines", 80, False))
if args.out:
    with open(args.out, "w") as f:
        json.dump({"what": "tools/exp_anchored.py: ms per call, medians of %d rounds of at least %.1f s per figure, (a) (b) (c) alternating; "
                           "spread = (max - min) / median of the rounds" % (args.rounds, args.window),
                   "device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
        f.write("\n")
