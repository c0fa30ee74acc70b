"""Shared by the tally_batch tests (test_tally_batch_cpu.py, test_tally_batch_gpu.py): the expected
text x keyword count matrix in CSR form, which is always derived from the ORACLE's scan of every text
alone (tests/batch_cases.oracle_batch_cut) and np.unique over text_id << 32 | keyword_id -- never from
the library's own scan --, the check of a result against it and the check that a workload cannot pass
trivially."""
import numpy as np

from tests.batch_cases import oracle_batch_cut


def expected(o, text, offsets):
    """(row_ptr, col, val) of the batch: uint64, uint32, uint64"""
    rec, tid, first = oracle_batch_cut(o, text, offsets)
    n_texts = len(offsets) - 1
    keys, counts = np.unique((tid.astype(np.uint64) << np.uint64(32)) | rec["keyword_id"].astype(np.uint64), return_counts=True)
    rows = (keys >> np.uint64(32)).astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_texts))]).astype(np.uint64)
    assert int(counts.sum()) == rec.size == int(first[-1])
    return row_ptr, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), counts.astype(np.uint64)


def check(got, want, what=""):
    """a TalliedBatch of numpy arrays cut to size against (row_ptr, col, val)"""
    row_ptr, col, val = want
    assert got.nnz == col.size, (what, "nnz", got.nnz, col.size)
    assert got.total == int(val.sum()), (what, "total", got.total, int(val.sum()))
    assert np.array_equal(np.asarray(got.row_ptr).astype(np.uint64), row_ptr), (what, "row_ptr")
    assert np.array_equal(np.asarray(got.col).astype(np.uint32), col), (what, "col")
    assert np.array_equal(np.asarray(got.val).astype(np.uint64), val), (what, "val")
    for t in range(row_ptr.size - 1):                                      # (implied by the equality above; said on its own)
        row = np.asarray(got.col[int(row_ptr[t]):int(row_ptr[t + 1])]).astype(np.int64)
        assert np.all(np.diff(row) > 0), (what, "row not ascending", t)


def dense(want, n_keywords):
    """the matrix as a dense numpy array of int64"""
    row_ptr, col, val = want
    m = np.zeros((row_ptr.size - 1, n_keywords), np.int64)
    rows = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr.astype(np.int64)))
    m[rows, col.astype(np.int64)] = val.astype(np.int64)
    return m


def nontrivial(o, text, offsets, want, window=None):
    """from the oracle alone: a row with two distinct keywords or more, a count of 2 or more, a text
    that is not empty with an empty row, a match of the concatenation that crosses a text boundary;
    with `window`: a text with records of ONE keyword that end in two different windows or more, so
    that the merge across windows has something to merge"""
    row_ptr, col, val = want
    off = np.asarray(offsets).astype(np.int64)
    lens = off[1:] - off[:-1]
    row_len = np.diff(row_ptr.astype(np.int64))
    whole = o.scan(text).size
    print("texts %d, rows with entries %d, widest row %d, entries %d, largest count %d, matches %d, in the concatenation %d" % (
        lens.size, int(np.count_nonzero(row_len)), int(row_len.max()), col.size, int(val.max()), int(val.sum()), whole))
    assert np.any(row_len >= 2)
    assert np.any(val >= 2)
    assert np.any((row_len == 0) & (lens > 0))
    assert whole > int(val.sum())
    if window is not None:
        per_key = np.unique(window_pairs(o, text, offsets, window)[:, 0], return_counts=True)[1]
        print("keys whose records end in two windows or more: %d" % int(np.count_nonzero(per_key >= 2)))
        assert np.any(per_key >= 2)


def window_pairs(o, text, offsets, window):
    """the distinct (text_id << 32 | keyword_id, window in which the record ends) of the batch, one per
    row: every one of them costs the device call a partial pair at the least"""
    rec, tid, first = oracle_batch_cut(o, text, offsets)
    key = (tid.astype(np.uint64) << np.uint64(32)) | rec["keyword_id"].astype(np.uint64)
    return np.unique(np.stack([key, rec["end_pos"] // np.uint64(window)], axis=1), axis=0)
