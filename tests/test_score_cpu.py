"""Weighted keyword scores per text without a GPU: acm_score_check, acm_score_matrix (the sequential
evaluation of a count matrix), acm_score_top and acm_score on a machine that takes the caller loop on
the host (ACM_SCAN_PATH_CPU_LOOP).  The expected answer is always the brute-force evaluation, with Python
integers modulo 2^64, of the ORACLE's count matrix (tests/score_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import score_class, weight
from tests.batch_cases import offsets_of, random_cuts
from tests.grep_cases import GREP_TEXTS
from tests.rules_cases import RULE_KEYWORDS
from tests.score_cases import EMPTY_COLUMN, EVERYWHERE, MODEL, NONE, check, check_top, nontrivial, wrapping_case
from tests.tally_batch_cases import expected
from tests.tally_cases import PATH_LOOP, byte_oracle, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
K = len(RULE_KEYWORDS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tallied(counts):
    return binding.TalliedBatch(counts[0], counts[1], counts[2], counts[1].size, int(counts[2].sum()))


@pytest.fixture(scope="module")
def case():
    """(count matrix of the oracle as a TalliedBatch, the model, the expected result) of the boundary set"""
    o = byte_oracle(RULE_KEYWORDS)
    text = np.frombuffer(b"".join(GREP_TEXTS), np.uint8)
    counts = expected(o, text, offsets_of(GREP_TEXTS))
    sm = binding.ScoreModel(MODEL)
    want = nontrivial(GREP_TEXTS, counts, sm, empty_column=EMPTY_COLUMN, everywhere=EVERYWHERE, ks=(1, 2), short_k=3)
    return _tallied(counts), sm, want


def test_the_boundary_model_is_the_worked_example_of_the_header(case):
    tallied, sm, want = case
    S = want.S
    assert want.n_kept == 46 and want.class_hits.tolist() == [5, 3, 10, 2, 0, 14, 11, 1]
    assert (S[11][0], S[7][0], S[8][0]) == (22, 8, 3)
    assert S[3][1] == 4 and [t for t in range(14) if want.keeps[t][1]] == [2, 3, 11]
    assert (S[7][2], S[11][2], S[1][2], S[9][2], S[10][2], S[0][2]) == (-1, -10, 3, 3, 3, 2)
    assert (S[3][3], S[11][3]) == (11, 21) and S[3][5] == 0
    assert (S[1][6], S[11][6]) == (2147483642, -2147483654)
    assert (S[11][7], S[2][7], S[3][7]) == (15, 5, 6) and [t for t in range(14) if want.keeps[t][7]] == [11]
    rows = np.diff(want.kept_ptr.astype(np.int64))
    assert rows.min() == 2 and rows.max() == 6
    assert all(want.best[t] == 2 for t in range(14) if len(GREP_TEXTS[t]) == 0)


def _check_rc(classes, n_keywords=K):
    sm = binding.ScoreModel(classes)
    return acm.lib().acm_score_check(*sm.args(), n_keywords)


def test_score_check_refuses_every_listed_case():
    assert _check_rc(MODEL) == 0
    assert _check_rc([]) == 0
    assert _check_rc([score_class([])]) == 0                                 # a class without terms
    assert _check_rc([score_class([weight(0, 0)])]) == 0                     # weight 0
    assert _check_rc([score_class([weight(0, 1, 0)])]) == E_ARG              # cap = 0
    assert _check_rc([score_class([weight(K, 1)])]) == E_ARG                 # a keyword id that is none
    assert _check_rc([score_class([weight(K - 1, 1)])]) == 0
    L = acm.lib()
    terms = np.array([(0, 1, NONE), (1, -1, 1)], binding.SCORE_TERM_DTYPE)
    two = np.zeros(2, np.int64)

    def call(class_ptr, n_classes=2, t=terms, b=two, th=two):
        cp = np.array(class_ptr, np.uint64)
        return L.acm_score_check(t.ctypes.data if t is not None else None, cp.ctypes.data, b.ctypes.data if b is not None else None,
                                 th.ctypes.data if th is not None else None, n_classes, K)
    assert call([0, 1, 2]) == 0 and call([0, 0, 2]) == 0 and call([0, 2, 2]) == 0
    assert call([0, 2, 1]) == E_ARG                                          # decreasing
    assert call([1, 1, 2]) == E_ARG                                          # does not begin with 0
    assert call([0, 1, 2], n_classes=1 << 31) == E_ARG
    assert call([0, 1, 1 << 31]) == E_ARG                                    # 2^31 terms
    assert call([0, 1, 2], t=None) == E_ARG and call([0, 1, 2], b=None) == E_ARG and call([0, 1, 2], th=None) == E_ARG
    assert L.acm_score_check(terms.ctypes.data, None, two.ctypes.data, two.ctypes.data, 2, K) == E_ARG


@pytest.mark.parametrize("k", [0, 1, 2, 3, 256])
def test_matrix_and_top_on_the_boundary_set(case, k):
    tallied, sm, want = case
    got = binding.score_matrix(tallied, sm, K)
    check(got, want, "acm_score_matrix")
    assert got.class_hits is None
    check_top(binding.score_top(got, sm.n_classes, k), want, k, ("acm_score_top", k))      # (256 > n_texts)
    dense = got.to_sparse_csr(sm.n_classes).to_dense().numpy()
    assert all(dense[t][c] == (want.S[t][c] if want.keeps[t][c] else 0) for t in range(want.n_texts) for c in range(sm.n_classes))


def _random_model(rng, n_keywords, n_classes):
    classes = []
    for c in range(n_classes):
        terms = [weight(int(rng.integers(0, n_keywords)), int(rng.integers(-9, 10)), [None, 1, 2, 5][int(rng.integers(0, 4))])
                 for _ in range(int(rng.integers(0, 6)))]
        classes.append(score_class(terms, bias=int(rng.integers(-3, 4)), threshold=int(rng.integers(-2, 6))))
    return classes


def test_matrix_and_top_on_a_random_model_over_random_cuts(novel_bytes):
    words = [b"the", b"he", b"and", b"an", b"of", b"t", b"her", b"e", b"is", b"was", b"zzzq"]
    o = byte_oracle(words)
    text = np.frombuffer(novel_bytes, np.uint8)[:60000]
    off = random_cuts(text.size, 300)
    counts = expected(o, text, off)
    sm = binding.ScoreModel(_random_model(np.random.default_rng(11), len(words), 40))
    texts = [bytes(text[int(off[t]):int(off[t + 1])]) for t in range(off.size - 1)]
    want = nontrivial(texts, counts, sm)
    got = binding.score_matrix(_tallied(counts), sm, len(words))
    check(got, want, "random")
    for k in (1, 7, 256):
        check_top(binding.score_top(got, sm.n_classes, k), want, k, ("random", k))


def test_matrix_and_top_wrap_modulo_two_to_the_64():
    tallied, sm, want = wrapping_case()
    got = binding.score_matrix(tallied, sm, 3)
    check(got, want, "wrapping")
    for k in (1, 3):
        check_top(binding.score_top(got, sm.n_classes, k), want, k, ("wrapping", k))


def _raw(tallied, sm, kept_ptr, kept_class, kept_score, cap, n, best=None, n_keywords=K, row_ptr=None, col=None):
    rp = tallied.row_ptr if row_ptr is None else row_ptr
    cl = tallied.col if col is None else col

    def p(a):
        return a.ctypes.data if a is not None else None
    return acm.lib().acm_score_matrix(rp.ctypes.data, cl.ctypes.data, tallied.val.ctypes.data, rp.size - 1, n_keywords, *sm.args(), p(kept_ptr),
                                      p(kept_class), p(kept_score), cap, C.byref(n) if n is not None else None, p(best))


def test_matrix_count_only_overflow_by_one_and_guards(case):
    tallied, sm, want = case
    n_texts, k = want.n_texts, want.n_kept
    n = C.c_uint64(99)
    kept_ptr = np.full(n_texts + 1, GUARD64, np.uint64)
    best = np.full(n_texts, GUARD32, np.uint32)
    assert _raw(tallied, sm, kept_ptr, None, None, 0, n, best) == 0          # no kept arrays: the call only counts
    assert n.value == k and np.array_equal(kept_ptr, want.kept_ptr) and np.all(best == GUARD32)
    cls, score = np.full(k - 1, GUARD32, np.uint32), np.full(k - 1, GUARD64, np.uint64).view(np.int64)
    kept_ptr[:] = GUARD64
    n.value = 99
    assert _raw(tallied, sm, kept_ptr, cls, score, k - 1, n, best) == E_OVERFLOW
    assert n.value == k and np.all(cls == GUARD32) and np.all(score.view(np.uint64) == GUARD64) and np.all(best == GUARD32)
    assert np.array_equal(kept_ptr, want.kept_ptr)
    cls, score = np.full(k + 3, GUARD32, np.uint32), np.full(k + 3, GUARD64, np.uint64).view(np.int64)
    assert _raw(tallied, sm, kept_ptr, cls, score, k, n, best) == 0
    assert np.array_equal(cls[:k], want.kept_class) and np.all(cls[k:] == GUARD32)
    assert np.array_equal(score[:k], want.kept_score) and np.all(score[k:].view(np.uint64) == GUARD64) and np.array_equal(best, want.best)
    assert _raw(tallied, sm, kept_ptr, cls, score, k, n, None) == 0          # best may be NULL


def test_matrix_arguments_and_no_text(case):
    tallied, sm, want = case
    n = C.c_uint64(0)
    kept_ptr, cls, score = np.zeros(want.n_texts + 1, np.uint64), np.zeros(want.n_kept, np.uint32), np.zeros(want.n_kept, np.int64)
    assert _raw(tallied, sm, kept_ptr, cls, score, cls.size, n) == 0
    down = tallied.row_ptr.copy()
    down[3], down[4] = tallied.row_ptr[4] + 1, tallied.row_ptr[3]
    assert down[3] > down[4] and _raw(tallied, sm, kept_ptr, cls, score, cls.size, n, row_ptr=down) == E_ARG
    one = tallied.row_ptr.copy()
    one[0] = 1
    assert _raw(tallied, sm, kept_ptr, cls, score, cls.size, n, row_ptr=one) == E_ARG
    high = tallied.col.copy()
    high[0] = K
    assert _raw(tallied, sm, kept_ptr, cls, score, cls.size, n, col=high) == E_ARG           # a col >= n_keywords
    assert _raw(tallied, sm, None, cls, score, cls.size, n) == E_ARG and _raw(tallied, sm, kept_ptr, cls, score, cls.size, None) == E_ARG
    assert _raw(tallied, binding.ScoreModel([score_class([weight(0, 1, 0)])]), kept_ptr, cls, score, cls.size, n) == E_ARG
    # no text at all: kept_ptr[0] = 0, nothing kept -- not even the always-classes; TOP of it is empty columns
    empty = binding.TalliedBatch(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0, 0)
    got = binding.score_matrix(empty, sm, K)
    assert got.n_kept == 0 and got.kept_ptr.tolist() == [0] and got.kept_class.size == 0 and got.best.size == 0
    top = binding.score_top(got, sm.n_classes, 3)
    assert not top.class_hits.any() and not top.top_n.any() and np.all(top.top_text == NONE) and not top.top_score.any()
    # texts without any keyword: the three always-classes with their biases, the best of them class 2
    got = binding.score_matrix(binding.TalliedBatch(np.zeros(4, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0, 0), sm, K)
    assert got.kept_ptr.tolist() == [0, 3, 6, 9] and got.kept_class.tolist() == [2, 5, 6] * 3 and got.kept_score.tolist() == [2, 0, -5] * 3
    assert got.best.tolist() == [2, 2, 2]


def test_top_arguments(case):
    tallied, sm, want = case
    got = binding.score_matrix(tallied, sm, K)
    L = acm.lib()
    hits, top_n, text, score = np.zeros(8, np.uint64), np.zeros(8, np.uint32), np.zeros(8 * 257, np.uint32), np.zeros(8 * 257, np.int64)

    def call(kept_ptr=got.kept_ptr, cls=got.kept_class, n_classes=8, k=3, n_texts=want.n_texts):
        return L.acm_score_top(kept_ptr.ctypes.data if kept_ptr is not None else None, cls.ctypes.data, got.kept_score.ctypes.data, n_texts, n_classes, k,
                               hits.ctypes.data, top_n.ctypes.data, text.ctypes.data, score.ctypes.data)
    assert call() == 0 and call(k=256) == 0
    assert call(k=257) == E_ARG and call(kept_ptr=None) == E_ARG and call(n_classes=7) == E_ARG        # class 7 is kept: no class then
    assert call(n_texts=1 << 31) == E_ARG and call(n_classes=1 << 31) == E_ARG
    down = got.kept_ptr.copy()
    down[2], down[3] = got.kept_ptr[3], got.kept_ptr[2]
    assert call(kept_ptr=down) == E_ARG
    one = got.kept_ptr.copy()
    one[0] = 1
    assert call(kept_ptr=one) == E_ARG
    assert L.acm_score_top(got.kept_ptr.ctypes.data, got.kept_class.ctypes.data, got.kept_score.ctypes.data, want.n_texts, 8, 0, hits.ctypes.data,
                           top_n.ctypes.data, None, None) == 0               # k = 0: the hits alone
    assert hits.tolist() == want.class_hits.tolist() and not top_n.any()


def test_machine_score_on_the_host_loop(case):
    """3-byte symbols: no GPU path takes the machine.  "us|hers" and "sh|e" cut a keyword by a text boundary"""
    tallied, sm, want = case
    m = acm.Machine(3)                                                   # ACM_CMP_DEFAULT over 3 bytes: the host loop
    for kw in RULE_KEYWORDS:
        buf = np.frombuffer(sym3(kw), np.uint8).copy()
        m._keep.append(buf)
        cur = C.c_void_p(m.L.acm_initiate(m.handle))
        for i in range(len(kw)):
            m.L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + 3 * i)
        m.L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    for k in (0, 2, 3):
        got = m.score([sym3(t) for t in GREP_TEXTS], sm, k=k)
        assert m.scan_path == PATH_LOOP
        check(got, want, ("Machine.score", k), k=k if k else None)
        assert got.total == tallied.total
    # through the C call: one entry too little room is an overflow that leaves the kept arrays, best and the top arrays alone; the path is recorded
    raw = np.frombuffer(b"".join(sym3(t) for t in GREP_TEXTS), np.uint8).copy()
    off = offsets_of(GREP_TEXTS)
    n_kept = want.n_kept
    kept_ptr, cls, score = np.zeros(off.size, np.uint64), np.full(n_kept - 1, GUARD32, np.uint32), np.full(n_kept - 1, 77, np.int64)
    best, hits, top_n = np.full(off.size - 1, GUARD32, np.uint32), np.full(8, GUARD64, np.uint64), np.full(8, GUARD32, np.uint32)
    text, tscore = np.full(16, GUARD32, np.uint32), np.full(16, 77, np.int64)
    n, total = C.c_uint64(99), C.c_uint64(99)
    rc = m.L.acm_score(m.handle, raw.ctypes.data, off.ctypes.data, off.size - 1, *sm.args(), kept_ptr.ctypes.data, cls.ctypes.data, score.ctypes.data,
                       n_kept - 1, C.byref(n), best.ctypes.data, 2, hits.ctypes.data, top_n.ctypes.data, text.ctypes.data, tscore.ctypes.data,
                       C.byref(total))
    assert rc == E_OVERFLOW and n.value == n_kept and total.value == tallied.total and np.array_equal(kept_ptr, want.kept_ptr)
    assert np.all(cls == GUARD32) and np.all(score == 77) and np.all(best == GUARD32) and np.all(hits == GUARD64) and np.all(top_n == GUARD32)
    assert np.all(text == GUARD32) and np.all(tscore == 77)
    empty = m.score([], sm, k=2)
    assert empty.kept_ptr.tolist() == [0] and not empty.class_hits.any()
    bad = binding.ScoreModel([score_class([weight(K, 1)])])
    assert m.L.acm_score(m.handle, raw.ctypes.data, off.ctypes.data, off.size - 1, *bad.args(), kept_ptr.ctypes.data, None, None, 0, C.byref(n), None, 0,
                         None, None, None, None, None) == E_ARG
    assert m.L.acm_score(m.handle, raw.ctypes.data, off.ctypes.data, off.size - 1, *sm.args(), kept_ptr.ctypes.data, None, None, 0, C.byref(n), None, 257,
                         None, None, None, None, None) == E_ARG


def test_plan_level_calls_refuse_before_they_touch_a_device():
    L = acm.lib()
    n = C.c_uint64(0)
    off = np.zeros(1, np.uint64)
    sm = binding.ScoreModel(MODEL)
    h = C.c_void_p()
    assert L.acm_gpu_score_create(None, *sm.args(), C.byref(h)) == E_ARG
    assert L.acm_gpu_score_matrix_tmp_bytes(None, None, 0) == 0 and L.acm_gpu_score_tmp_bytes(None, None, 16, 16, 16, 0, 0, 16, 0) == 0
    assert L.acm_gpu_score_top_tmp_bytes(None, 16, 8) == 0
    assert L.acm_gpu_score_matrix_device(None, None, None, None, None, 0, None, None, None, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_score_top_device(None, None, None, None, 0, 0, 0, 0, None, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_score_device(None, None, None, 0, None, 0, 16, 16, 16, None, None, None, 0, None, None, 0, None, None, None, None, None, None, None,
                                  None, 0, None) == E_ARG
    assert L.acm_gpu_score_host(None, None, off.ctypes.data, 0, *sm.args(), off.ctypes.data, None, None, 0, C.byref(n), None, 0, None, None, None, None,
                                None) == E_ARG
    assert L.acm_gpu_score_info(None, None) == E_ARG
    L.acm_gpu_score_destroy(None)


NAMES = ("acm_score_check", "acm_score_matrix", "acm_score_top", "acm_gpu_score_create", "acm_gpu_score_destroy", "acm_gpu_score_info",
         "acm_gpu_score_matrix_tmp_bytes", "acm_gpu_score_matrix_device", "acm_gpu_score_top_tmp_bytes", "acm_gpu_score_top_device",
         "acm_gpu_score_tmp_bytes", "acm_gpu_score_device", "acm_gpu_score_host", "acm_score")


def test_library_exports_the_score_symbols():
    L = acm.lib()
    for name in NAMES:
        assert name in binding.EXPORTS and getattr(L, name) is not None, name


def test_the_header_declares_exactly_these_and_acm_gpu_h_includes_it():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acm_score.h")).read(), flags=re.S)      # comments mention functions too
    assert set(re.findall(r"\b(acm_[a-z0-9_]+)\s*\(", text)) == set(NAMES)
    assert '#include "acm_score.h"' in open(os.path.join(ROOT, "include", "acm_gpu.h")).read().split("#endif")[-1]


def test_header_compiles_as_c11_and_every_declared_function_links(tmp_path):
    """include/acm_score.h behind acm_gpu.h, and first of all"""
    for k, head in enumerate(('#include "aho_corasick.h"\n#include "acm_gpu.h"\n#include "acm_score.h"\n', '#include "acm_score.h"\n')):
        src = head + "int main(void){" + "".join("(void)%s;" % n for n in NAMES) + "return sizeof (ACMScoreTerm) == 12 ? 0 : 1;}\n"
        exe = str(tmp_path / ("link_check_%d" % k))
        p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe,
                            "-L", os.path.dirname(acm.library_path()), "-lac75_amd", "-Wl,-rpath," + os.path.dirname(acm.library_path())],
                           input=src.encode(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode()
        assert subprocess.run([exe]).returncode == 0
