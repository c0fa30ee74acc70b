"""Shared by the co-occurrence tests (test_cooccur_cpu.py, test_cooccur_gpu.py): the worked example of
include/acm_cooccur.h, the expected matrix -- always the brute force of the definition over the ORACLE's count
matrix (tests/tally_batch_cases.expected), never over the library's own counts --, the check of a result against it
and the check that a workload cannot pass trivially."""
import numpy as np

from aho_corasick_1975_amd import binding
from tests.grep_cases import GREP_TEXTS
from tests.rules_cases import RULE_KEYWORDS

PRODUCT, DIAGONAL = 1, 2
ALL_FLAGS = (0, DIAGONAL, PRODUCT, PRODUCT | DIAGONAL)
MASK = (1 << 64) - 1
EXAMPLE_KEYWORDS, EXAMPLE_TEXTS = RULE_KEYWORDS, GREP_TEXTS
_PLAIN = {(0, 1): 2, (0, 2): 3, (0, 3): 4, (1, 2): 1, (1, 3): 2, (2, 3): 3}
_PLAIN_DIAGONAL = {(0, 0): 5, (1, 1): 2, (2, 2): 3, (3, 3): 7}
_PRODUCT = {(0, 1): 9, (0, 2): 10, (0, 3): 22, (1, 2): 4, (1, 3): 11, (2, 3): 11}
_PRODUCT_DIAGONAL = {(0, 0): 20, (1, 1): 5, (2, 2): 6, (3, 3): 33}
# the tables of the header: flags -> (cross, nnz, co_ptr, {(a, b): value})
EXAMPLE = {
    0: (15, 6, [0, 3, 5, 6, 6, 6], _PLAIN),
    DIAGONAL: (32, 10, [0, 4, 7, 9, 10, 10], {**_PLAIN, **_PLAIN_DIAGONAL}),
    PRODUCT: (15, 6, [0, 3, 5, 6, 6, 6], _PRODUCT),
    PRODUCT | DIAGONAL: (32, 10, [0, 4, 7, 9, 10, 10], {**_PRODUCT, **_PRODUCT_DIAGONAL}),
}
# row_limit = 3 under flags 0: text 11 (four keywords) is skipped
EXAMPLE_LIMIT3 = (9, 5, 1, {(0, 1): 1, (0, 2): 2, (0, 3): 3, (1, 3): 1, (2, 3): 2})


class Expected:
    """the matrix as co_ptr (uint64), co_col (uint32), co_val (uint64), with nnz, cross, skipped and flags"""

    def __init__(self, co_ptr, co_col, co_val, cross, skipped, flags):
        self.co_ptr, self.co_col, self.co_val = np.asarray(co_ptr, np.uint64), np.asarray(co_col, np.uint32), np.asarray(co_val, np.uint64)
        self.nnz, self.cross, self.skipped, self.flags, self.n_keywords = int(self.co_col.size), int(cross), int(skipped), int(flags), int(self.co_ptr.size) - 1

    def entries(self):
        """{(a, b): value}"""
        return {(a, int(self.co_col[e])): int(self.co_val[e]) for a in range(self.n_keywords) for e in range(int(self.co_ptr[a]), int(self.co_ptr[a + 1]))}


def _of_entries(entries, n_keywords, cross, skipped, flags):
    ptr, col, val = [0], [], []
    rows = [[] for _ in range(n_keywords)]
    for (a, b) in sorted(entries):
        rows[a].append((b, entries[(a, b)]))
    for r in rows:
        col += [b for b, _ in r]
        val += [v for _, v in r]
        ptr.append(len(col))
    return Expected(ptr, col, val, cross, skipped, flags)


def brute_force(counts, n_keywords, flags=0, row_limit=0):
    """the Expected of the count matrix `counts` = (row_ptr, col, val): the definition, text by text and pair by pair, modulo 2^64"""
    row_ptr, col, val = counts
    entries, cross, skipped = {}, 0, 0
    for t in range(len(row_ptr) - 1):
        row = [(int(col[e]), int(val[e])) for e in range(int(row_ptr[t]), int(row_ptr[t + 1]))]
        if row_limit and len(row) > row_limit:
            skipped += 1
            continue
        for i, (a, ca) in enumerate(row):
            for b, cb in row[i if flags & DIAGONAL else i + 1:]:
                assert a < n_keywords and b < n_keywords and a <= b
                entries[(a, b)] = (entries.get((a, b), 0) + (ca * cb if flags & PRODUCT else 1)) & MASK
                cross += 1
    return _of_entries(entries, n_keywords, cross, skipped, flags)


def add_expected(a, b):
    """the entrywise sum modulo 2^64 of two Expected over b's keywords: the brute force of ADD"""
    assert a.n_keywords <= b.n_keywords
    entries = a.entries()
    for key, v in b.entries().items():
        entries[key] = (entries.get(key, 0) + v) & MASK
    return _of_entries(entries, b.n_keywords, a.cross + b.cross, a.skipped + b.skipped, b.flags)


def tallied_of(counts):
    """the count matrix (row_ptr, col, val) as a TalliedBatch of numpy arrays"""
    return binding.TalliedBatch(np.asarray(counts[0], np.uint64), np.asarray(counts[1], np.uint32), np.asarray(counts[2], np.uint64), int(len(counts[1])),
                                int(np.asarray(counts[2], np.uint64).sum()))


def cooccurred_of(e):
    """an Expected as a Cooccurred of numpy arrays (the input of an ADD)"""
    return binding.Cooccurred(e.co_ptr.copy(), e.co_col.copy(), e.co_val.copy(), e.nnz, e.cross, e.skipped, e.flags)


def cut_rows(counts, lo, hi):
    """rows [lo, hi) of a count matrix as a count matrix of their own"""
    row_ptr, col, val = counts
    a, b = int(row_ptr[lo]), int(row_ptr[hi])
    return (np.asarray(row_ptr[lo:hi + 1], np.uint64) - np.uint64(a)), np.asarray(col[a:b]), np.asarray(val[a:b])


def matrix_of(rows):
    """a count matrix from a list of {keyword: count} rows"""
    row_ptr, col, val = [0], [], []
    for row in rows:
        col += sorted(row)
        val += [row[k] for k in sorted(row)]
        row_ptr.append(len(col))
    return np.array(row_ptr, np.uint64), np.array(col, np.uint32), np.array(val, np.uint64)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def check(got, want, what="", counts=True):
    """a Cooccurred (numpy arrays, or device tensors) against an Expected; counts: cross and skipped as well"""
    n = want.nnz
    assert got.nnz == n, (what, "nnz", got.nnz, n)
    ptr = _host(got.co_ptr).astype(np.uint64)
    assert np.array_equal(ptr, want.co_ptr), (what, "co_ptr", ptr.tolist()[:20], want.co_ptr.tolist()[:20])
    col = _host(got.co_col)[:n].view(np.uint32) if n else np.zeros(0, np.uint32)
    val = _host(got.co_val)[:n].astype(np.uint64) if n else np.zeros(0, np.uint64)
    assert np.array_equal(col, want.co_col), (what, "co_col", col.tolist()[:40], want.co_col.tolist()[:40])
    assert np.array_equal(val, want.co_val), (what, "co_val", val.tolist()[:40], want.co_val.tolist()[:40])
    for a in range(want.n_keywords):                                       # (implied by the equality above; said on its own)
        ids = col[int(ptr[a]):int(ptr[a + 1])].astype(np.int64)
        assert np.all(np.diff(ids) > 0), (what, "row not strictly ascending", a)
        assert np.all(ids >= a) if want.flags & DIAGONAL else np.all(ids > a), (what, "an entry below the triangle", a)
    if counts:
        assert got.cross == want.cross and got.skipped == want.skipped, (what, "cross, skipped", got.cross, want.cross, got.skipped, want.skipped)
        if not want.flags & PRODUCT:
            assert sum(int(v) for v in val) == got.cross, (what, "the values do not sum to cross")


def nontrivial(counts, want):
    """from the oracle alone: entries at all, a value >= 2, an empty row, a text with >= 3 keywords"""
    row_len = np.diff(np.asarray(counts[0]).astype(np.int64))
    rows = np.diff(want.co_ptr.astype(np.int64))
    print("texts %d, keywords %d, entries %d, pair instances %d, skipped %d, greatest value %d, empty rows %d, widest text %d" % (
        row_len.size, want.n_keywords, want.nnz, want.cross, want.skipped, int(want.co_val.max()) if want.nnz else 0, int(np.count_nonzero(rows == 0)),
        int(row_len.max())))
    assert want.nnz > 0
    assert int(want.co_val.max()) >= 2
    assert np.any(rows == 0)
    assert np.any(row_len >= 3)
    return want
