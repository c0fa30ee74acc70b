"""Shared by the grep tests (test_grep_cpu.py, test_grep_gpu.py): the expected answer, which is always
derived from the ORACLE's scan of every text alone (tests/batch_cases.py: hits = np.diff (first)) and
numpy -- never from the library's own scan --, and the check that a workload cannot pass trivially."""
import numpy as np

from tests.batch_cases import TEXTS, oracle_batch_cut

# batch_cases.TEXTS with one text more that no keyword of batch_cases.KEYWORDS matches, between its two
# empty texts in the middle (every boundary of TEXTS stays what it was: "us|hers", "sh|e", the empty
# texts at the front, in the middle and at the end)
GREP_TEXTS = TEXTS[:5] + [b"on top"] + TEXTS[5:]


def oracle_hits(o, text, offsets):
    """hits[t] = first[t + 1] - first[t] of the oracle's batch"""
    first = oracle_batch_cut(o, text, offsets)[2]
    return np.diff(first.astype(np.int64)).astype(np.uint64)


def nontrivial(o, text, offsets, hits):
    """from the oracle alone: a text that is not empty without a hit, two distinct non-zero hit counts,
    a match of the concatenation that crosses a text boundary, both KEPT sets non-empty"""
    off = np.asarray(offsets).astype(np.int64)
    lens = off[1:] - off[:-1]
    whole = o.scan(text).size
    distinct = np.unique(hits[hits > 0])
    print("texts %d, empty %d, with a hit %d, distinct non-zero counts %d, matches %d, in the concatenation %d" % (
        hits.size, int(np.count_nonzero(lens == 0)), int(np.count_nonzero(hits)), distinct.size, int(hits.sum()), whole))
    assert np.any((hits == 0) & (lens > 0))
    assert distinct.size >= 2
    assert whole > int(hits.sum())
    assert np.any(hits > 0) and np.any(hits == 0)


def expected(text, offsets, hits, invert, sym_size=None):
    """(kept, out_offsets, out as raw bytes) in numpy; `text` an array of symbols, or raw bytes with sym_size"""
    t = np.ascontiguousarray(text)
    sb = int(sym_size) if sym_size is not None else t.itemsize
    raw = t.reshape(-1).view(np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    keep = (hits == 0) if invert else (hits > 0)
    kept = np.flatnonzero(keep).astype(np.uint32)
    lens = (off[1:] - off[:-1])[keep]
    out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    parts = [raw[off[t] * sb:off[t + 1] * sb] for t in kept]
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    assert out.size == int(out_off[-1]) * sb
    return kept, out_off, out


def check(got, hits, want, sym_size, what=""):
    """a Grepped of numpy arrays against (kept, out_offsets, out bytes)"""
    kept, out_off, out = want
    assert np.array_equal(got.hits, hits), (what, "hits")
    assert got.n_kept == kept.size and np.array_equal(got.kept, kept), (what, "kept")
    assert got.total == int(hits.sum()), (what, "total")
    assert np.array_equal(got.out_offsets, out_off), (what, "out_offsets")
    assert got.out_symbols == int(out_off[-1]), (what, "out_symbols")
    if got.out is not None:
        assert np.array_equal(np.ascontiguousarray(got.out).reshape(-1).view(np.uint8), out), (what, "out")
