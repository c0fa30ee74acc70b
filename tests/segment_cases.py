"""Shared by the segmentation tests (test_segment_cpu.py, test_segment_gpu.py): the expected answer, which
is always the definition of SEGMENT (include/acm_segment.h) in plain Python over the ORACLE's records --
never the library's own scan --, the exhaustive minimum over all tilings that checks the definition's own
cost, and the worked examples of the header."""
import numpy as np

from oracle import pyoracle as po
from tests.select_cases import assert_tiling, oracle_records, random_case
from tests.tally_cases import byte_oracle


def define(records, cost, gap, pos_lo=None, n=None):
    """SEGMENT by its definition, position by position: best[0] = 0; best[p] = min (best[p - 1] + gap, min
    over the records that end at p - 1 of best[start] + cost[kw]); backwards from p = n: of the records
    that end at p - 1 and attain best[p] the longest (then the smaller keyword_id), p = its start, else
    p - 1.  Returns (records, total cost over [pos_lo, pos_lo + n))."""
    rec = np.asarray(records)
    if rec.size == 0:
        return np.zeros(0, po.RECORD_DTYPE), 0
    end = rec["end_pos"].astype(object)
    length = rec["length"].astype(object)
    kw = rec["keyword_id"]
    start = end + 1 - length
    if pos_lo is None:
        pos_lo = int(min(start))
    if n is None:
        n = int(max(end)) + 1 - pos_lo
    ends_at = {}
    for i in range(rec.size):
        ends_at.setdefault(int(end[i]) - pos_lo + 1, []).append(i)
    best = [0] * (n + 1)
    for p in range(1, n + 1):
        b = best[p - 1] + gap
        for i in ends_at.get(p, ()):
            b = min(b, best[int(start[i]) - pos_lo] + int(cost[kw[i]]))
        best[p] = b
    take, p = [], n
    while p > 0:
        m = [i for i in ends_at.get(p, ()) if best[int(start[i]) - pos_lo] + int(cost[kw[i]]) == best[p]]
        if m:
            i = min(m, key=lambda i: (-int(length[i]), int(kw[i])))
            take.append(i)
            p = int(start[i]) - pos_lo
        else:
            p -= 1
    out = rec[np.array(take[::-1], np.int64)].astype(po.RECORD_DTYPE) if take else np.zeros(0, po.RECORD_DTYPE)
    assert_tiling(out)
    assert tiling_cost(out, cost, gap, n) == best[n]
    return out, best[n]


def tiling_cost(sel, cost, gap, n):
    return int(sum(int(cost[k]) for k in sel["keyword_id"])) + gap * (n - int(sel["length"].astype(np.int64).sum()))


def exhaustive_minimum(records, cost, gap, n):
    """the least cost over ALL tilings of at most 14 records: every subset in which no two share a symbol"""
    rec = np.asarray(records)
    assert rec.size <= 14
    end = rec["end_pos"].astype(np.int64)
    start = end + 1 - rec["length"].astype(np.int64)
    least = gap * n
    for mask in range(1, 1 << rec.size):
        idx = [i for i in range(rec.size) if mask >> i & 1]
        idx.sort(key=lambda i: start[i])
        if all(start[b] > end[a] for a, b in zip(idx, idx[1:])):
            least = min(least, tiling_cost(rec[idx], cost, gap, n))
    return least


def n_groups(records):
    """maximal groups of records chained by shared symbols, from the records alone"""
    rec = np.asarray(records)
    if rec.size == 0:
        return 0
    end = rec["end_pos"].astype(np.int64)
    start = end + 1 - rec["length"].astype(np.int64)
    order = np.argsort(start, kind="stable")
    groups, reach = 0, None
    for i in order:
        if reach is None or start[i] > reach:
            groups += 1
            reach = end[i]
        reach = max(reach, end[i])
    return groups


# the header's worked examples: (text, keywords, costs, gap, expected records or None, total cost)
EXAMPLES = [
    (b"ushers", [b"he", b"she", b"his", b"hers"], [1, 1, 1, 1], 2, [(5, 4, 3)], 5),
    (b"abcd", [b"ab", b"abc", b"cd"], [1, 1, 1], 10, [(1, 2, 0), (3, 2, 2)], 2),
    (b"a" * 1001, [b"a", b"aa"], [2, 4], 2, [(0, 1, 0)] + [(2 * k, 2, 1) for k in range(1, 501)], 2002),
    (b"a" * 1000, [b"a", b"aa", b"aaa"], [5, 6, 100], 7, [(2 * k + 1, 2, 1) for k in range(500)], 3000),
]


def example(k):
    """(oracle's records, cost array, gap, expected selection, total, text, keywords) of worked example k"""
    text, keywords, cost, gap, rows, total = EXAMPLES[k]
    rec = oracle_records(byte_oracle(keywords), text)
    want = np.array(rows, po.RECORD_DTYPE)
    return rec, np.array(cost, np.uint32), gap, want, total, text, keywords


def random_cases(seed=1975, count=200):
    """the generator family of test_select_cpu.py with costs and gap_cost drawn from 0 .. 7:
    (keywords, text, cost, gap) per case"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        keywords, text = random_case(rng, 8, 6, int(rng.integers(1, 301)))
        cost = rng.integers(0, 8, size=len(keywords)).astype(np.uint32)
        yield keywords, text, cost, int(rng.integers(0, 8))
