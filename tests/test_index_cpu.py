"""The inverted index of a batch without a GPU: acm_index_matrix (the sequential transposition of a count
matrix), acm_index_concat and acm_index on a machine that takes the caller loop on the host
(ACM_SCAN_PATH_CPU_LOOP).  The expected answer is always the brute-force transposition of the ORACLE's
count matrix (tests/index_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import offsets_of
from tests.index_cases import (EXAMPLE_KEYWORDS, EXAMPLE_NNZ, EXAMPLE_POSTINGS, EXAMPLE_PTR, EXAMPLE_TEXTS, EXAMPLE_TOTAL, brute_force, check,
                               concat_expected, cut_rows, indexed_of, nontrivial, tallied_of)
from tests.tally_batch_cases import expected
from tests.tally_cases import PATH_LOOP, byte_oracle, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
K = len(EXAMPLE_KEYWORDS)
N = len(EXAMPLE_TEXTS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP_BASE = (1 << 32) - N


@pytest.fixture(scope="module")
def case():
    """(the oracle's count matrix, its brute-force index) of the worked example"""
    o = byte_oracle(EXAMPLE_KEYWORDS)
    text = np.frombuffer(b"".join(EXAMPLE_TEXTS), np.uint8)
    counts = expected(o, text, offsets_of(EXAMPLE_TEXTS))
    return counts, nontrivial(counts, brute_force(counts, K))


def test_the_worked_example_of_the_header(case):
    """the oracle's matrix, transposed by brute force, is the table of the header; so is substring counting"""
    counts, want = case
    assert want.post_ptr.tolist() == EXAMPLE_PTR and want.nnz == EXAMPLE_NNZ and want.total == EXAMPLE_TOTAL
    for k, kw in enumerate(EXAMPLE_KEYWORDS):
        lo, hi = int(want.post_ptr[k]), int(want.post_ptr[k + 1])
        assert list(zip(want.post_text[lo:hi].tolist(), want.post_count[lo:hi].tolist())) == EXAMPLE_POSTINGS[kw], kw
        by_hand = [(t, sum(1 for i in range(len(s)) if s.startswith(kw, i))) for t, s in enumerate(EXAMPLE_TEXTS)]
        assert [(t, c) for t, c in by_hand if c] == EXAMPLE_POSTINGS[kw], kw
    assert want.df.tolist() == [5, 2, 3, 7, 0]
    got = binding.index_matrix(tallied_of(counts), K)
    check(got, want, "acm_index_matrix")
    assert [x.tolist() for x in got.postings(1)] == [[3, 11], [1, 2]] and got.postings(4)[0].size == 0
    dense = got.to_sparse_csr(N).to_dense().numpy()
    assert all(dense[k][t] == dict(EXAMPLE_POSTINGS[kw]).get(t, 0) for k, kw in enumerate(EXAMPLE_KEYWORDS) for t in range(N))
    # more keywords than the matrix knows: empty lists behind
    check(binding.index_matrix(tallied_of(counts), K + 3), brute_force(counts, K + 3), "n_keywords + 3")


def _random_matrix(rng, n_texts, n_keywords, empty_cols):
    row_ptr, col, val = [0], [], []
    live = [k for k in range(n_keywords) if k not in empty_cols]
    for t in range(n_texts):
        if rng.random() < 0.25:
            picks = []
        else:
            picks = sorted(rng.choice(live, size=int(rng.integers(1, 9)), replace=False).tolist())
        col += picks
        val += [int(rng.integers(1, 1 << 40)) for _ in picks]
        row_ptr.append(len(col))
    return np.array(row_ptr, np.uint64), np.array(col, np.uint32), np.array(val, np.uint64)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_matrices_with_empty_rows_and_columns(seed):
    rng = np.random.default_rng(seed)
    counts = _random_matrix(rng, 200, 50, {0, 17, 49})
    assert np.any(np.diff(counts[0].astype(np.int64)) == 0)
    for base in (0, 1000):
        want = nontrivial(counts, brute_force(counts, 50, base))
        check(binding.index_matrix(tallied_of(counts), 50, base), want, ("random", seed, base))


def _raw(counts, post_ptr, post_text, post_count, cap, n, n_keywords=K, base=0, row_ptr=None, col=None, n_texts=None):
    rp = counts[0] if row_ptr is None else row_ptr
    cl = counts[1] if col is None else col

    def p(a):
        return a.ctypes.data if a is not None else None
    return acm.lib().acm_index_matrix(p(rp), p(cl), counts[2].ctypes.data, rp.size - 1 if n_texts is None else n_texts, n_keywords, base, p(post_ptr),
                                      p(post_text), p(post_count), cap, C.byref(n) if n is not None else None)


def test_matrix_arguments(case):
    counts, want = case
    n = C.c_uint64(0)
    ptr, text, count = np.zeros(K + 1, np.uint64), np.zeros(want.nnz, np.uint32), np.zeros(want.nnz, np.uint64)
    assert _raw(counts, ptr, text, count, text.size, n) == 0
    down = counts[0].copy()
    down[3], down[4] = counts[0][4] + 1, counts[0][3]
    assert down[3] > down[4] and _raw(counts, ptr, text, count, text.size, n, row_ptr=down) == E_ARG
    one = counts[0].copy()
    one[0] = 1
    assert _raw(counts, ptr, text, count, text.size, n, row_ptr=one) == E_ARG
    high = counts[1].copy()
    high[0] = K
    assert _raw(counts, ptr, text, count, text.size, n, col=high) == E_ARG                  # a col >= n_keywords
    assert _raw(counts, ptr, text, count, text.size, n, n_keywords=K - 1) == 0              # (qux occurs nowhere: four keywords do)
    assert _raw(counts, ptr, text, count, text.size, n, n_keywords=K - 2) == E_ARG          # (s does)
    assert _raw(counts, None, text, count, text.size, n) == E_ARG and _raw(counts, ptr, text, count, text.size, None) == E_ARG
    assert _raw(counts, ptr, text, count, text.size, n, n_keywords=1 << 32) == E_ARG
    assert _raw(counts, ptr, text, count, text.size, n, n_texts=1 << 31) == E_ARG
    assert _raw(counts, ptr, text, count, 1 << 31, n) == E_ARG
    # text_base + n_texts <= 2^32: the last base that fits, and one more
    assert _raw(counts, ptr, text, count, text.size, n, base=TOP_BASE) == 0
    assert text.max() == (1 << 32) - 1 - 2 and np.array_equal(text, brute_force(counts, K, TOP_BASE).post_text)
    assert _raw(counts, ptr, text, count, text.size, n, base=TOP_BASE + 1) == E_ARG
    assert _raw(counts, ptr, text, count, text.size, n, base=(1 << 64) - 1) == E_ARG
    # no text at all
    got = binding.index_matrix(binding.TalliedBatch(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0, 0), K)
    assert got.nnz == 0 and got.post_ptr.tolist() == [0] * (K + 1)


def test_matrix_count_only_overflow_by_one_and_guards(case):
    counts, want = case
    k = want.nnz
    n = C.c_uint64(99)
    ptr = np.full(K + 1, GUARD64, np.uint64)
    assert _raw(counts, ptr, None, None, 0, n) == 0                          # NULL: the call only counts
    assert n.value == k and np.array_equal(ptr, want.post_ptr)
    text, count = np.full(k, GUARD32, np.uint32), np.full(k, GUARD64, np.uint64)
    ptr[:] = GUARD64
    n.value = 99
    assert _raw(counts, ptr, text, None, k, n) == 0 and np.all(text == GUARD32)  # one of the two NULL: counts as well
    assert _raw(counts, ptr, text, count, k - 1, n) == E_OVERFLOW
    assert n.value == k and np.all(text == GUARD32) and np.all(count == GUARD64) and np.array_equal(ptr, want.post_ptr)
    text, count = np.full(k + 3, GUARD32, np.uint32), np.full(k + 3, GUARD64, np.uint64)
    assert _raw(counts, ptr, text, count, k, n) == 0
    assert np.array_equal(text[:k], want.post_text) and np.all(text[k:] == GUARD32)
    assert np.array_equal(count[:k], want.post_count) and np.all(count[k:] == GUARD64) and np.array_equal(ptr, want.post_ptr)


def test_concat_of_the_halves_is_the_whole(case):
    counts, want = case
    a = brute_force(cut_rows(counts, 0, 7), K)
    b = brute_force(cut_rows(counts, 7, N), K, 7)
    assert a.nnz > 0 and b.nnz > 0 and a.nnz + b.nnz == want.nnz
    A = binding.index_matrix(tallied_of(cut_rows(counts, 0, 7)), K)
    B = binding.index_matrix(tallied_of(cut_rows(counts, 7, N)), K, 7)
    check(A, a, "texts 0..6")
    check(B, b, "texts 7..13 at base 7")
    check(binding.index_concat(A, B), want, "the halves")
    check(binding.index_concat(indexed_of(a), indexed_of(b)), concat_expected(a, b), "the brute force agrees")


def test_concat_is_associative_over_three_parts(case):
    counts, want = case
    parts = [binding.index_matrix(tallied_of(cut_rows(counts, lo, hi)), K, lo) for lo, hi in ((0, 3), (3, 9), (9, N))]
    assert all(p.nnz > 0 for p in parts)
    left = binding.index_concat(binding.index_concat(parts[0], parts[1]), parts[2])
    right = binding.index_concat(parts[0], binding.index_concat(parts[1], parts[2]))
    check(left, want, "(a b) c")
    check(right, want, "a (b c)")


def test_concat_with_a_dictionary_that_grew(case):
    """A over 4 keywords (he, she, hers, s), B over all 5: keyword ids are first-insertion ranks"""
    counts, want = case
    first = cut_rows(counts, 0, 7)
    assert int(first[1].max()) < 4
    A = binding.index_matrix(tallied_of(first), 4)
    B = binding.index_matrix(tallied_of(cut_rows(counts, 7, N)), K, 7)
    assert A.n_keywords == 4 and B.n_keywords == 5
    check(binding.index_concat(A, B), want, "4 keywords, then 5")
    # and a keyword that only B has entries for
    grown = brute_force((np.array([0, 1, 2], np.uint64), np.array([5, 0], np.uint32), np.array([9, 1], np.uint64)), 6, N)
    whole = concat_expected(want, grown)
    assert whole.df.tolist() == [6, 2, 3, 7, 0, 1]
    check(binding.index_concat(indexed_of(want), indexed_of(grown)), whole, "5 keywords, then 6")


def _concat_raw(a, b, out_ptr, out_text, out_count, cap, n, n_a=None, n_b=None, a_ptr=None, b_ptr=None):
    def p(x):
        return x.ctypes.data if x is not None else None
    ap = a.post_ptr if a_ptr is None else a_ptr
    bp = b.post_ptr if b_ptr is None else b_ptr
    return acm.lib().acm_index_concat(p(ap), p(a.post_text), p(a.post_count), a.n_keywords if n_a is None else n_a, p(bp), p(b.post_text), p(b.post_count),
                                      b.n_keywords if n_b is None else n_b, p(out_ptr), p(out_text), p(out_count), cap, C.byref(n) if n is not None else None)


def test_concat_arguments_overflow_and_count_only(case):
    counts, want = case
    a = brute_force(cut_rows(counts, 0, 7), K)
    b = brute_force(cut_rows(counts, 7, N), K, 7)
    k = want.nnz
    n = C.c_uint64(99)
    ptr, text, count = np.full(K + 1, GUARD64, np.uint64), np.full(k, GUARD32, np.uint32), np.full(k, GUARD64, np.uint64)
    assert _concat_raw(a, b, ptr, None, None, 0, n) == 0 and n.value == k and np.array_equal(ptr, want.post_ptr)
    ptr[:] = GUARD64
    assert _concat_raw(a, b, ptr, text, count, k - 1, n) == E_OVERFLOW
    assert n.value == k and np.array_equal(ptr, want.post_ptr) and np.all(text == GUARD32) and np.all(count == GUARD64)
    assert _concat_raw(a, b, ptr, text, count, k, n) == 0 and np.array_equal(text, want.post_text) and np.array_equal(count, want.post_count)
    # a boundary violation: B's first id must lie ABOVE A's last -- at base 0 B's `hers` begins with text 0, A's ends with 2
    low = brute_force(cut_rows(counts, 7, N), K, 0)
    assert _concat_raw(a, low, ptr, text, count, k, n) == E_ARG
    same = brute_force(cut_rows(counts, 0, 7), K)                            # equal ids are not above either
    assert _concat_raw(a, same, ptr, text, count, k, n) == E_ARG
    assert _concat_raw(b, a, ptr, text, count, k, n) == E_ARG                # the wrong way round
    assert _concat_raw(a, b, ptr, text, count, k, n, n_a=K, n_b=K - 1) == E_ARG         # n_keywords_a > n_keywords_b
    down = a.post_ptr.copy()
    down[1], down[2] = a.post_ptr[2], a.post_ptr[1]
    assert down[1] > down[2] and _concat_raw(a, b, ptr, text, count, k, n, a_ptr=down) == E_ARG
    one = b.post_ptr.copy()
    one[0] = 1
    assert _concat_raw(a, b, ptr, text, count, k, n, b_ptr=one) == E_ARG
    bdown = b.post_ptr.copy()
    bdown[3], bdown[4] = b.post_ptr[4], b.post_ptr[3]
    assert bdown[3] > bdown[4] and _concat_raw(a, b, ptr, text, count, k, n, b_ptr=bdown) == E_ARG
    assert _concat_raw(a, b, None, text, count, k, n) == E_ARG and _concat_raw(a, b, ptr, text, count, k, None) == E_ARG


def test_machine_index_on_the_host_loop(case):
    """3-byte symbols: no GPU path takes the machine.  "us|hers" and "sh|e" cut a keyword by a text boundary"""
    counts, want = case
    m = acm.Machine(3)                                                   # ACM_CMP_DEFAULT over 3 bytes: the host loop
    for kw in EXAMPLE_KEYWORDS:
        buf = np.frombuffer(sym3(kw), np.uint8).copy()
        m._keep.append(buf)
        cur = C.c_void_p(m.L.acm_initiate(m.handle))
        for i in range(len(kw)):
            m.L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + 3 * i)
        m.L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    texts = [sym3(t) for t in EXAMPLE_TEXTS]
    got = m.index(texts)
    assert m.scan_path == PATH_LOOP
    check(got, want, "Machine.index")
    check(m.index(texts, n_keywords=K + 2, text_base=TOP_BASE), brute_force(counts, K + 2, TOP_BASE), "Machine.index, more keywords, the last base")
    # through the C call: one entry too little room is an overflow that leaves the lists alone; the path is recorded
    raw = np.frombuffer(b"".join(texts), np.uint8).copy()
    off = offsets_of(EXAMPLE_TEXTS)
    k = want.nnz
    ptr, text, count = np.zeros(K + 1, np.uint64), np.full(k - 1, GUARD32, np.uint32), np.full(k - 1, GUARD64, np.uint64)
    n, total = C.c_uint64(99), C.c_uint64(99)

    def call(n_keywords=K, base=0, cap=k - 1):
        return m.L.acm_index(m.handle, raw.ctypes.data, off.ctypes.data, off.size - 1, base, ptr.ctypes.data, n_keywords, text.ctypes.data, count.ctypes.data,
                             cap, C.byref(n), C.byref(total))
    assert call() == E_OVERFLOW and n.value == k and total.value == want.total and np.array_equal(ptr, want.post_ptr)
    assert np.all(text == GUARD32) and np.all(count == GUARD64)
    assert call(n_keywords=K - 1) == E_ARG and call(base=TOP_BASE + 1) == E_ARG and call(n_keywords=1 << 32) == E_ARG
    empty = m.index([])
    assert empty.nnz == 0 and empty.post_ptr.tolist() == [0] * (K + 1)


def test_plan_level_calls_refuse_before_they_touch_a_device():
    L = acm.lib()
    n = C.c_uint64(0)
    off = np.zeros(1, np.uint64)
    assert L.acm_gpu_index_matrix_tmp_bytes(None, 0, 0, 0) == 0 and L.acm_gpu_index_concat_tmp_bytes(None, 0) == 0
    assert L.acm_gpu_index_tmp_bytes(None, 16, 16, 16, 0, 0, 0, 0) == 0
    assert L.acm_gpu_index_matrix_device(None, None, None, None, 0, 0, 0, None, None, None, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_index_concat_device(None, None, None, None, 0, None, None, None, 0, None, None, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_index_device(None, None, 0, None, 0, 16, 16, 16, 0, 0, None, None, None, 0, None, None, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_index_host(None, None, off.ctypes.data, 0, 0, off.ctypes.data, 0, None, None, 0, C.byref(n), None) == E_ARG


NAMES = ("acm_index_matrix", "acm_index_concat", "acm_gpu_index_matrix_tmp_bytes", "acm_gpu_index_matrix_device", "acm_gpu_index_concat_tmp_bytes",
         "acm_gpu_index_concat_device", "acm_gpu_index_tmp_bytes", "acm_gpu_index_device", "acm_gpu_index_host", "acm_index")


def test_library_exports_exactly_the_index_symbols():
    L = acm.lib()
    for name in NAMES:
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
    nm = subprocess.run(["nm", "-D", "--defined-only", acm.library_path()], capture_output=True, check=True).stdout.decode()
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    assert set(s for s in exported if "index" in s and s.startswith("acm_")) == set(NAMES)


def test_the_header_declares_exactly_these_and_acm_gpu_h_includes_it():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acm_index.h")).read(), flags=re.S)      # comments mention functions too
    assert set(re.findall(r"\b(acm_[a-z0-9_]+)\s*\(", text)) == set(NAMES)
    assert '#include "acm_index.h"' in open(os.path.join(ROOT, "include", "acm_gpu.h")).read().split("#endif")[-1]


def test_header_compiles_as_c11_and_every_declared_function_links(tmp_path):
    """include/acm_index.h behind acm_gpu.h, and first of all"""
    for k, head in enumerate(('#include "aho_corasick.h"\n#include "acm_gpu.h"\n#include "acm_index.h"\n', '#include "acm_index.h"\n')):
        src = head + "int main(void){" + "".join("(void)%s;" % n for n in NAMES) + "return 0;}\n"
        exe = str(tmp_path / ("link_check_%d" % k))
        p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe,
                            "-L", os.path.dirname(acm.library_path()), "-lac75_amd", "-Wl,-rpath," + os.path.dirname(acm.library_path())],
                           input=src.encode(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode()
        assert subprocess.run([exe]).returncode == 0
