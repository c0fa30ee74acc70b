"""Shared by the score tests (test_score_cpu.py, test_score_gpu.py): the boundary model over the
boundary keywords (the worked example of include/acm_score.h), the expected kept matrix, BEST and TOP
-- always the brute-force evaluation, with Python integers reduced modulo 2^64, of the ORACLE's count
matrix (tests/tally_batch_cases.expected and dense), never of the library's own counts --, the check of
a result against it and the check that a workload cannot pass trivially."""
import numpy as np

from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import score_class, weight
from tests.rules_cases import HE, HERS, NEVER, S, SHE

NO_CAP, NONE = binding.ACM_SCORE_NO_CAP, binding.ACM_SCORE_NONE
M64 = (1 << 64) - 1

MODEL = [
    score_class([weight(HE, 3), weight(HERS, 5)]),                                           # 0  a plain sum
    score_class([weight(S, 2, 2)], threshold=3),                                              # 1  saturation; a three-way tie for TOP
    score_class([weight(HE, -4), weight(S, 1)], bias=2),                                      # 2  an always-class that he switches off
    score_class([weight(SHE, 1, 1), weight(SHE, 10)]),                                        # 3  one keyword twice; a column of 2
    score_class([weight(NEVER, 7)]),                                                          # 4  a keyword no text holds: an empty column
    score_class([weight(HE, 1), weight(SHE, -1)], threshold=0),                               # 5  cancelling; an always-class kept everywhere
    score_class([weight(HERS, -(1 << 31)), weight(S, (1 << 31) - 1, 1)], bias=-5, threshold=-5),  # 6  the extreme weights
    score_class([weight(HE, 3), weight(S, 1, 3)], threshold=7),                               # 7  kept in one text alone
]
EMPTY_COLUMN, EVERYWHERE = 4, 5
ALWAYS = (2, 5, 6)


def signed(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def model_of(model):
    return model if isinstance(model, binding.ScoreModel) else binding.ScoreModel(model)


def scores_of_rows(rows, model):
    """S[t][c] as Python integers (two's complement modulo 2^64) from rows = one {keyword: count} per text"""
    sm = model_of(model)
    out = []
    for row in rows:
        line = []
        for c in range(sm.n_classes):
            s = int(sm.bias[c])
            for k, w, cap in sm.terms[int(sm.class_ptr[c]):int(sm.class_ptr[c + 1])].tolist():
                cnt = row.get(k, 0)
                s += w * (cnt if cap == NO_CAP else min(cnt, cap))
            line.append(signed(s))
        out.append(line)
    return out, sm


def rows_of(want):
    """one {keyword: count} per text of a count matrix (row_ptr, col, val)"""
    row_ptr, col, val = want
    return [{int(col[e]): int(val[e]) for e in range(int(row_ptr[t]), int(row_ptr[t + 1]))} for t in range(len(row_ptr) - 1)]


class Expected:
    """the kept matrix, BEST and (top (k)) TOP of a score matrix S (lists of Python integers)"""

    def __init__(self, S, sm):
        self.S, self.n_classes, self.n_texts = S, sm.n_classes, len(S)
        th = [int(x) for x in sm.threshold]
        self.keeps = [[S[t][c] >= th[c] for c in range(sm.n_classes)] for t in range(len(S))]
        ptr, cls, score, best = [0], [], [], []
        for t in range(len(S)):
            row = [(c, S[t][c]) for c in range(sm.n_classes) if self.keeps[t][c]]
            cls += [c for c, _ in row]
            score += [s for _, s in row]
            ptr.append(len(cls))
            best.append(min(row, key=lambda cs: (-cs[1], cs[0]))[0] if row else NONE)
        self.kept_ptr, self.kept_class = np.array(ptr, np.uint64), np.array(cls, np.uint32)
        self.kept_score, self.best = np.array(score, np.int64), np.array(best, np.uint32)
        self.n_kept = len(cls)
        self.class_hits = np.array([sum(self.keeps[t][c] for t in range(len(S))) for c in range(sm.n_classes)], np.uint64)

    def top(self, k):
        """(top_n, top_text [n_classes, k], top_score [n_classes, k])"""
        top_n = np.minimum(self.class_hits, k).astype(np.uint32)
        text, score = np.full((self.n_classes, k), NONE, np.uint32), np.zeros((self.n_classes, k), np.int64)
        for c in range(self.n_classes):
            column = sorted(((-self.S[t][c], t) for t in range(self.n_texts) if self.keeps[t][c]))[:k]
            for j, (neg, t) in enumerate(column):
                text[c, j], score[c, j] = t, -neg
        return top_n, text, score


def expected_scored(want, model):
    """the Expected of the oracle's count matrix `want` = (row_ptr, col, val): the brute force"""
    S, sm = scores_of_rows(rows_of(want), model)
    return Expected(S, sm)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def check(got, want, what="", k=None, best=True):
    """a Scored (numpy arrays, or device tensors) against an Expected; k: the top arrays too"""
    n = want.n_kept
    assert got.n_kept == n, (what, "n_kept", got.n_kept, n)
    assert np.array_equal(_host(got.kept_ptr).astype(np.uint64), want.kept_ptr), (what, "kept_ptr")
    cls, score = _host(got.kept_class)[:n].astype(np.uint32), _host(got.kept_score)[:n].astype(np.int64)
    assert np.array_equal(cls, want.kept_class), (what, "kept_class", cls.tolist(), want.kept_class.tolist())
    assert np.array_equal(score, want.kept_score), (what, "kept_score", score.tolist(), want.kept_score.tolist())
    for t in range(want.n_texts):                                          # (implied by the equality above; said on its own)
        assert np.all(np.diff(cls[int(want.kept_ptr[t]):int(want.kept_ptr[t + 1])].astype(np.int64)) > 0), (what, "row not ascending", t)
    if best:
        assert got.best is not None and np.array_equal(_host(got.best).view(np.uint32), want.best), (what, "best", _host(got.best).tolist(), want.best.tolist())
    if k is not None:
        check_top(got, want, k, what)


def check_top(got, want, k, what=""):
    top_n, text, score = want.top(k)
    assert np.array_equal(_host(got.class_hits).astype(np.uint64), want.class_hits), (what, "class_hits", _host(got.class_hits).tolist())
    assert np.array_equal(_host(got.top_n).view(np.uint32), top_n), (what, "top_n", _host(got.top_n).tolist(), top_n.tolist())
    assert np.array_equal(_host(got.top_text).view(np.uint32).reshape(text.shape), text), (what, "top_text", k, _host(got.top_text).tolist(), text.tolist())
    assert np.array_equal(_host(got.top_score).astype(np.int64).reshape(score.shape), score), (what, "top_score", k)


def nontrivial(texts, want, model, empty_column=None, everywhere=None, ks=(), short_k=None):
    """from the oracle alone: every class but `empty_column` is kept somewhere, every class but `everywhere` leaves a
    text out, a row keeps two classes or more, an always-class is kept on an empty text and switched off on a non-empty
    one, a capped term has a text with count > cap; for every k of `ks` some column has a tie that k cuts through; with
    short_k some column is shorter than short_k and some column is empty"""
    rows = rows_of(want)
    S, sm = scores_of_rows(rows, model)
    e = Expected(S, sm)
    lens = [len(t) for t in texts]
    per_row = np.diff(e.kept_ptr.astype(np.int64))
    print("texts %d, classes %d, kept %d, per class %s, rows of %d to %d" % (len(texts), sm.n_classes, e.n_kept, e.class_hits.tolist(),
                                                                          int(per_row.min()), int(per_row.max())))
    for c in range(sm.n_classes if empty_column is not None or everywhere is not None else 0):
        assert (e.class_hits[c] == 0) == (c == empty_column), ("kept nowhere", c)
        assert (e.class_hits[c] == len(texts)) == (c == everywhere), ("kept everywhere", c)
    assert np.any(e.class_hits > 0) and np.any(e.class_hits < len(texts))
    assert np.any(per_row >= 2)
    always = [c for c in range(sm.n_classes) if int(sm.bias[c]) >= int(sm.threshold[c])]
    assert any(lens[t] == 0 and e.keeps[t][c] for t in range(len(texts)) for c in always)
    assert any(lens[t] > 0 and not e.keeps[t][c] for t in range(len(texts)) for c in always)
    assert any(cap != NO_CAP and any(row.get(k, 0) > cap for row in rows) for k, w, cap in sm.terms.tolist())
    for k in ks:
        cut = False
        for c in range(sm.n_classes):
            column = sorted((-S[t][c], t) for t in range(len(texts)) if e.keeps[t][c])
            cut |= len(column) > k and column[k - 1][0] == column[k][0]
        assert cut, ("no tie that k cuts through", k)
    if short_k:
        assert np.any((e.class_hits > 0) & (e.class_hits < short_k)) and np.any(e.class_hits == 0)
    return e


def wrapping_case():
    """(a caller's own count matrix as a TalliedBatch, the model, the Expected): counts of 2^40 and 2^63 under weights of
    +-(2^31 - 1), so that products and sums wrap; the expected values are Python integers reduced modulo 2^64"""
    big = (1 << 31) - 1
    rows = [{0: 1 << 40, 1: 1 << 63}, {}, {1: (1 << 63) + 3, 2: 5}, {0: (1 << 64) - 1, 1: 1 << 62, 2: 1 << 40}]
    model = [score_class([weight(0, big), weight(1, big)], bias=7, threshold=0),
             score_class([weight(0, -big), weight(1, -big), weight(2, big, 3)], bias=-1, threshold=-(1 << 40)),
             score_class([weight(1, big, 2), weight(1, 2)], bias=(1 << 63) - 1, threshold=1),          # bias + 2 * 2^63 + ... wraps past the top
             score_class([weight(2, -big)], bias=-(1 << 63), threshold=-(1 << 63)),                    # INT64_MIN: every text
             score_class([weight(0, 1), weight(0, -1)], bias=0, threshold=0)]
    row_ptr, col, val = [0], [], []
    for row in rows:
        for k in sorted(row):
            col.append(k)
            val.append(row[k])
        row_ptr.append(len(col))
    S, sm = scores_of_rows(rows, model)
    want = Expected(S, sm)
    assert any(abs(s) > (1 << 62) for line in S for s in line) and 0 < want.n_kept < len(rows) * sm.n_classes
    # the sums do wrap: the exact value of some kept pair lies outside 64 bits
    exact = [int(sm.bias[c]) + sum(w * (row.get(k, 0) if cap == binding.ACM_SCORE_NO_CAP else min(row.get(k, 0), cap))
                                   for k, w, cap in sm.terms[int(sm.class_ptr[c]):int(sm.class_ptr[c + 1])].tolist())
             for row in rows for c in range(sm.n_classes)]
    assert any(not -(1 << 63) <= x < (1 << 63) for x in exact)
    t = binding.TalliedBatch(np.array(row_ptr, np.uint64), np.array(col, np.uint32), np.array(val, np.uint64), len(col), 0)
    return t, sm, want
