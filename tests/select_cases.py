"""Shared by the selection tests (test_select_cpu.py, test_select_gpu.py): the expected answer, which is
always the definition of SELECT (include/acm_gpu.h) in plain Python over the ORACLE's records -- never
the library's own scan --, and the check that a case cannot pass trivially."""
import numpy as np

from oracle import pyoracle as po


def greedy(records):
    """SELECT by its definition: p = the smallest position; among the records with start >= p those
    with the smallest start, of those the longest (then the smaller keyword_id); emit it, p = its
    end_pos + 1; until no record has start >= p.  Quadratic wording made linear by one sort: with the
    records in (start, -length, keyword_id) order the record taken is the first with start >= p."""
    rec = np.asarray(records)
    if rec.size == 0:
        return np.zeros(0, po.RECORD_DTYPE)
    end = rec["end_pos"].astype(np.int64)
    length = rec["length"].astype(np.int64)
    kw = rec["keyword_id"].astype(np.int64)
    start = end + 1 - length
    order = np.lexsort((kw, -length, start))
    take, p = [], None
    for i in order:
        if p is None or start[i] >= p:
            take.append(i)
            p = end[i] + 1
    out = rec[np.array(take, np.int64)].astype(po.RECORD_DTYPE)
    assert_tiling(out)
    return out


def assert_tiling(sel):
    """canonical order, no two records share a symbol"""
    end = sel["end_pos"].astype(np.int64)
    start = end + 1 - sel["length"].astype(np.int64)
    assert np.all(start[1:] > end[:-1]), "selected records overlap or are out of order"


def oracle_records(o, text):
    return o.scan(text) if len(text) else np.zeros(0, po.RECORD_DTYPE)


def nontrivial(all_records, sel):
    """from the oracle alone: something is selected and something is left out"""
    print("records %d, selected %d" % (len(all_records), len(sel)))
    assert 0 < len(sel) < len(all_records), (len(sel), len(all_records))


def random_case(rng, max_keywords, max_len, n_text):
    """(keywords, text) over an alphabet of 2-3 symbols: up to max_keywords distinct keywords of 1 to
    max_len symbols"""
    alpha = int(rng.integers(2, 4))
    words = set()
    for _ in range(int(rng.integers(2, max_keywords + 1))):
        words.add(bytes(rng.integers(97, 97 + alpha, size=int(rng.integers(1, max_len + 1)), dtype=np.uint8)))
    text = bytes(rng.integers(97, 97 + alpha, size=n_text, dtype=np.uint8))
    return sorted(words), text
