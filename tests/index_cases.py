"""Shared by the index tests (test_index_cpu.py, test_index_gpu.py, test_index_streams_gpu.py): the
worked example of include/acm_index.h, the expected inverted index -- always the brute-force
transposition of the ORACLE's count matrix (tests/tally_batch_cases.expected), never of the library's own
counts --, the check of a result against it and the check that a workload cannot pass trivially."""
import numpy as np

from aho_corasick_1975_amd import binding
from tests.grep_cases import GREP_TEXTS
from tests.rules_cases import RULE_KEYWORDS

EXAMPLE_KEYWORDS, EXAMPLE_TEXTS = RULE_KEYWORDS, GREP_TEXTS
# the table of the header: keyword -> [(text, count)]
EXAMPLE_POSTINGS = {
    b"he": [(2, 1), (3, 1), (7, 1), (8, 1), (11, 4)],
    b"she": [(3, 1), (11, 2)],
    b"hers": [(2, 1), (7, 1), (11, 2)],
    b"s": [(1, 1), (2, 2), (3, 3), (7, 1), (9, 1), (10, 1), (11, 4)],
    b"qux": [],
}
EXAMPLE_PTR, EXAMPLE_NNZ, EXAMPLE_TOTAL = [0, 5, 7, 10, 17, 17], 17, 28


class Expected:
    """the index as post_ptr (uint64), post_text (uint32), post_count (uint64), with nnz, total and df"""

    def __init__(self, post_ptr, post_text, post_count, text_base=0):
        self.post_ptr, self.post_text = np.asarray(post_ptr, np.uint64), np.asarray(post_text, np.uint32)
        self.post_count, self.text_base = np.asarray(post_count, np.uint64), text_base
        self.nnz, self.total, self.n_keywords = int(self.post_text.size), int(self.post_count.sum()), int(self.post_ptr.size) - 1
        self.df = np.diff(self.post_ptr.astype(np.int64))


def brute_force(want, n_keywords, text_base=0):
    """the Expected of the count matrix `want` = (row_ptr, col, val): for every keyword, every text in order"""
    row_ptr, col, val = want
    lists = [[] for _ in range(n_keywords)]
    for t in range(len(row_ptr) - 1):
        for e in range(int(row_ptr[t]), int(row_ptr[t + 1])):
            lists[int(col[e])].append((text_base + t, int(val[e])))
    ptr, text, count = [0], [], []
    for lst in lists:
        text += [t for t, _ in lst]
        count += [c for _, c in lst]
        ptr.append(len(text))
    return Expected(ptr, text, count, text_base)


def concat_expected(a, b):
    """per keyword a's list, then b's (two Expected): the brute force of CONCAT"""
    ptr, text, count = [0], [], []
    for k in range(b.n_keywords):
        if k < a.n_keywords:
            lo, hi = int(a.post_ptr[k]), int(a.post_ptr[k + 1])
            text += a.post_text[lo:hi].tolist()
            count += a.post_count[lo:hi].tolist()
        lo, hi = int(b.post_ptr[k]), int(b.post_ptr[k + 1])
        text += b.post_text[lo:hi].tolist()
        count += b.post_count[lo:hi].tolist()
        ptr.append(len(text))
    return Expected(ptr, text, count, a.text_base)


def tallied_of(want):
    """the count matrix (row_ptr, col, val) as a TalliedBatch of numpy arrays"""
    return binding.TalliedBatch(np.asarray(want[0], np.uint64), np.asarray(want[1], np.uint32), np.asarray(want[2], np.uint64), int(len(want[1])),
                                int(np.asarray(want[2], np.uint64).sum()))


def indexed_of(e):
    """an Expected as an Indexed of numpy arrays (the input of a CONCAT)"""
    return binding.Indexed(e.post_ptr.copy(), e.post_text.copy(), e.post_count.copy(), e.nnz, e.total, e.text_base)


def cut_rows(want, lo, hi):
    """rows [lo, hi) of a count matrix as a count matrix of their own"""
    row_ptr, col, val = want
    a, b = int(row_ptr[lo]), int(row_ptr[hi])
    return (np.asarray(row_ptr[lo:hi + 1], np.uint64) - np.uint64(a)), np.asarray(col[a:b]), np.asarray(val[a:b])


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def check(got, want, what="", total=True):
    """an Indexed (numpy arrays, or device tensors) against an Expected"""
    n = want.nnz
    assert got.nnz == n, (what, "nnz", got.nnz, n)
    ptr = _host(got.post_ptr).astype(np.uint64)
    assert np.array_equal(ptr, want.post_ptr), (what, "post_ptr", ptr.tolist()[:20], want.post_ptr.tolist()[:20])
    text = _host(got.post_text)[:n].view(np.uint32) if n else np.zeros(0, np.uint32)
    count = _host(got.post_count)[:n].astype(np.uint64) if n else np.zeros(0, np.uint64)
    assert np.array_equal(text, want.post_text), (what, "post_text", text.tolist()[:40], want.post_text.tolist()[:40])
    assert np.array_equal(count, want.post_count), (what, "post_count", count.tolist()[:40], want.post_count.tolist()[:40])
    assert np.all(count > 0), (what, "a count of 0")
    for k in range(want.n_keywords):                                       # (implied by the equality above; said on its own)
        lst = text[int(ptr[k]):int(ptr[k + 1])].astype(np.int64)
        assert np.all(np.diff(lst) > 0), (what, "list not strictly ascending", k)
    assert np.array_equal(_host(got.df()).astype(np.int64), want.df), (what, "df")
    if total:
        assert got.total == want.total, (what, "total", got.total, want.total)


def nontrivial(counts, want, longest=None, fast=None, wide=None):
    """from the oracle alone: entries at all, a list with df >= 2, a text with >= 2 keywords, an empty list; with
    `longest` (the value of ACM_GPU_INDEX_LIST) how many lists either form has to put in order must be `fast` / `wide`"""
    row_len = np.diff(np.asarray(counts[0]).astype(np.int64))
    print("texts %d, keywords %d, entries %d, total %d, longest list %d, lists of two or more %d, empty lists %d, widest row %d" % (
        row_len.size, want.n_keywords, want.nnz, want.total, int(want.df.max()), int(np.count_nonzero(want.df >= 2)),
        int(np.count_nonzero(want.df == 0)), int(row_len.max())))
    assert want.nnz > 0
    assert np.any(want.df >= 2)
    assert np.any(row_len >= 2)
    assert np.any(want.df == 0)
    if longest is not None:
        assert forms_of(want, longest) == (fast, wide), (forms_of(want, longest), fast, wide)
    return want


def forms_of(want, longest):
    """(lists the fast form puts in order, lists the wide form does) with ACM_GPU_INDEX_LIST = longest"""
    return int(np.count_nonzero((want.df >= 1) & (want.df <= longest))), int(np.count_nonzero(want.df > longest))
