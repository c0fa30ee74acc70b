"""The keyword co-occurrence matrix of a batch without a GPU: acm_cooccur_matrix (the sequential definition on a
count matrix), acm_cooccur_add and acm_cooccur on a machine that takes the caller loop on the host
(ACM_SCAN_PATH_CPU_LOOP), the header and the binding's list.  The expected answer is always the brute force of the
definition over the ORACLE's count matrix (tests/cooccur_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import offsets_of
from tests.cooccur_cases import (ALL_FLAGS, DIAGONAL, EXAMPLE, EXAMPLE_KEYWORDS, EXAMPLE_LIMIT3, EXAMPLE_TEXTS, MASK, PRODUCT, add_expected, brute_force,
                                 check, cooccurred_of, cut_rows, matrix_of, nontrivial, tallied_of)
from tests.tally_batch_cases import expected
from tests.tally_cases import PATH_LOOP, byte_oracle, sym3
from tests.test_binding_signatures import PROTOTYPE, c_class, signature

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
K = len(EXAMPLE_KEYWORDS)
N = len(EXAMPLE_TEXTS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "acm_cooccur.h")


@pytest.fixture(scope="module")
def counts():
    """the oracle's count matrix of the worked example"""
    o = byte_oracle(EXAMPLE_KEYWORDS)
    text = np.frombuffer(b"".join(EXAMPLE_TEXTS), np.uint8)
    return expected(o, text, offsets_of(EXAMPLE_TEXTS))


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_the_worked_example_of_the_header(counts, flags):
    """the oracle's matrix under the brute force of the definition is the table of the header; so is substring counting"""
    cross, nnz, ptr, entries = EXAMPLE[flags]
    want = nontrivial(counts, brute_force(counts, K, flags))
    assert (want.cross, want.nnz, want.co_ptr.tolist(), want.entries()) == (cross, nnz, ptr, entries) and want.skipped == 0
    by_hand = [[sum(1 for i in range(len(s)) if s.startswith(kw, i)) for kw in EXAMPLE_KEYWORDS] for s in EXAMPLE_TEXTS]
    for (a, b), v in entries.items():
        assert v == sum(r[a] * r[b] if flags & PRODUCT else 1 for r in by_hand if r[a] and r[b]), (a, b)
    got = binding.cooccur_matrix(tallied_of(counts), flags, n_keywords=K)
    check(got, want, ("acm_cooccur_matrix", flags))
    assert got.flags == flags and got.n_keywords == K
    assert [x.tolist() for x in got.row(1)] == [[b for (a, b) in sorted(entries) if a == 1], [entries[k] for k in sorted(entries) if k[0] == 1]]
    assert got.value(3, 0) == got.value(0, 3) == entries[(0, 3)] and got.value(0, 4) == 0 and got.value(4, 4) == 0
    dense = got.to_sparse_csr(K).to_dense().numpy()
    assert all(dense[a][b] == entries.get((a, b), 0) for a in range(K) for b in range(K))
    # more keywords than the matrix knows: empty rows behind
    check(binding.cooccur_matrix(tallied_of(counts), flags, n_keywords=K + 3), brute_force(counts, K + 3, flags), "n_keywords + 3")
    # n_keywords None: one more than the greatest id the matrix holds (qux occurs nowhere)
    assert binding.cooccur_matrix(tallied_of(counts), flags).n_keywords == K - 1


def test_row_limit_three_skips_the_text_with_four_keywords(counts):
    cross, nnz, skipped, entries = EXAMPLE_LIMIT3
    want = brute_force(counts, K, 0, 3)
    assert (want.cross, want.nnz, want.skipped, want.entries()) == (cross, nnz, skipped, entries)
    check(binding.cooccur_matrix(tallied_of(counts), 0, 3, K), want, "row_limit 3")
    for flags in ALL_FLAGS:
        for limit in (1, 2, 3, 4, 1 << 63):
            want = brute_force(counts, K, flags, limit)
            assert want.skipped == {1: 4, 2: 4, 3: 1}.get(limit, 0)
            check(binding.cooccur_matrix(tallied_of(counts), flags, limit, K), want, ("row_limit", flags, limit))


def _random_matrix(rng, n_texts, n_keywords, empty_cols, most=9):
    live = [k for k in range(n_keywords) if k not in empty_cols]
    rows = []
    for t in range(n_texts):
        picks = [] if rng.random() < 0.25 else rng.choice(live, size=int(rng.integers(1, most)), replace=False).tolist()
        rows.append({k: int(rng.integers(1, 1 << 40)) for k in picks})
    return matrix_of(rows)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_matrices_with_empty_rows_and_columns(seed):
    rng = np.random.default_rng(seed)
    m = _random_matrix(rng, 200, 30, {0, 17, 29})
    assert np.any(np.diff(m[0].astype(np.int64)) == 0)
    for flags in ALL_FLAGS:
        for limit in (0, 5):
            want = nontrivial(m, brute_force(m, 30, flags, limit))
            assert (want.skipped > 0) == (limit > 0)
            check(binding.cooccur_matrix(tallied_of(m), flags, limit, 30), want, ("random", seed, flags, limit))


def test_products_of_counts_near_2_to_the_64_wrap_as_python_says():
    big = [1 << 63, (1 << 64) - 1, (1 << 63) + 1, 3]
    m = matrix_of([{0: big[0], 1: big[1], 2: big[2]}, {0: big[1], 1: big[1]}, {1: big[0], 2: big[0], 3: big[3]}, {}, {0: 3, 1: 5, 2: 7},
                   {4: 1 << 32, 5: 1 << 32}])
    for flags in (PRODUCT, PRODUCT | DIAGONAL):
        want = brute_force(m, 7, flags)
        assert want.entries()[(0, 1)] == (big[0] * big[1] + big[1] * big[1] + 15) & MASK
        assert want.entries()[(4, 5)] == 0 and max(want.entries().values()) > 1 << 63      # (an entry whose sum wrapped to 0 stays an entry)
        check(binding.cooccur_matrix(tallied_of(m), flags, 0, 7), want, ("wrap", flags))


def _raw(counts, co_ptr, co_col, co_val, cap, n, n_keywords=K, flags=0, limit=0, row_ptr=None, col=None, n_texts=None, cross=None, skipped=None):
    rp = counts[0] if row_ptr is None else row_ptr
    cl = counts[1] if col is None else col

    def p(a):
        return a.ctypes.data if a is not None else None
    return acm.lib().acm_cooccur_matrix(p(rp), p(cl), counts[2].ctypes.data, rp.size - 1 if n_texts is None else n_texts, n_keywords, flags, limit, p(co_ptr),
                                        p(co_col), p(co_val), cap, C.byref(n) if n is not None else None, C.byref(cross) if cross is not None else None,
                                        C.byref(skipped) if skipped is not None else None)


def test_matrix_arguments(counts):
    want = brute_force(counts, K)
    n = C.c_uint64(0)
    ptr, col, val = np.zeros(K + 1, np.uint64), np.zeros(want.nnz, np.uint32), np.zeros(want.nnz, np.uint64)
    assert _raw(counts, ptr, col, val, col.size, n) == 0
    down = counts[0].copy()
    down[3], down[4] = counts[0][4] + 1, counts[0][3]
    assert down[3] > down[4] and _raw(counts, ptr, col, val, col.size, n, row_ptr=down) == E_ARG
    one = counts[0].copy()
    one[0] = 1
    assert _raw(counts, ptr, col, val, col.size, n, row_ptr=one) == E_ARG
    high = counts[1].copy()
    high[0] = K
    assert _raw(counts, ptr, col, val, col.size, n, col=high) == E_ARG                    # a col >= n_keywords
    twice = counts[1].copy()
    twice[2] = twice[1]
    assert _raw(counts, ptr, col, val, col.size, n, col=twice) == E_ARG                   # a row that repeats a keyword
    assert _raw(counts, ptr, col, val, col.size, n, n_keywords=K - 1) == 0                # (qux occurs nowhere: four keywords do)
    assert _raw(counts, ptr, col, val, col.size, n, n_keywords=K - 2) == E_ARG            # (s does)
    assert _raw(counts, None, col, val, col.size, n) == E_ARG and _raw(counts, ptr, col, val, col.size, None) == E_ARG
    assert _raw(counts, ptr, col, val, col.size, n, n_keywords=1 << 32) == E_ARG
    assert _raw(counts, ptr, col, val, col.size, n, n_texts=1 << 31) == E_ARG
    assert _raw(counts, ptr, col, val, 1 << 31, n) == E_ARG                               # a room of 2^31 entries
    assert _raw(counts, ptr, col, val, col.size, n, flags=4) == E_ARG and _raw(counts, ptr, col, val, col.size, n, flags=1 << 31) == E_ARG
    assert _raw(counts, ptr, None, None, 0, n, flags=3) == 0 and n.value == 10
    # no text at all
    got = binding.cooccur_matrix(binding.TalliedBatch(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0, 0), n_keywords=K)
    assert (got.nnz, got.cross, got.skipped) == (0, 0, 0) and got.co_ptr.tolist() == [0] * (K + 1)
    with pytest.raises(acm.ACMError):
        binding.cooccur_matrix(tallied_of(counts), 8, n_keywords=K)


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_matrix_count_only_overflow_by_one_and_guards(counts, flags):
    want = brute_force(counts, K, flags, 3)
    k = want.nnz
    n, cross, skipped = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
    ptr = np.full(K + 1, GUARD64, np.uint64)
    assert _raw(counts, ptr, None, None, 0, n, flags=flags, limit=3, cross=cross, skipped=skipped) == 0     # NULL: the call only counts
    assert (n.value, cross.value, skipped.value) == (k, want.cross, 1) and np.array_equal(ptr, want.co_ptr)
    col, val = np.full(k, GUARD32, np.uint32), np.full(k, GUARD64, np.uint64)
    ptr[:] = GUARD64
    n.value = cross.value = skipped.value = 99
    assert _raw(counts, ptr, col, None, k, n, flags=flags, limit=3) == 0 and np.all(col == GUARD32)         # one of the two NULL: counts as well
    assert _raw(counts, ptr, col, val, k - 1, n, flags=flags, limit=3, cross=cross, skipped=skipped) == E_OVERFLOW
    assert (n.value, cross.value, skipped.value) == (k, want.cross, 1)
    assert np.all(col == GUARD32) and np.all(val == GUARD64) and np.array_equal(ptr, want.co_ptr)
    col, val = np.full(k + 3, GUARD32, np.uint32), np.full(k + 3, GUARD64, np.uint64)
    assert _raw(counts, ptr, col, val, k, n, flags=flags, limit=3) == 0
    assert np.array_equal(col[:k], want.co_col) and np.all(col[k:] == GUARD32)
    assert np.array_equal(val[:k], want.co_val) and np.all(val[k:] == GUARD64) and np.array_equal(ptr, want.co_ptr)


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_add_of_the_halves_is_the_whole(counts, flags):
    want = brute_force(counts, K, flags)
    a, b = brute_force(cut_rows(counts, 0, 7), K, flags), brute_force(cut_rows(counts, 7, N), K, flags)
    assert a.nnz > 0 and b.nnz > 0 and set(a.entries()) & set(b.entries()) and want.nnz < a.nnz + b.nnz
    A = binding.cooccur_matrix(tallied_of(cut_rows(counts, 0, 7)), flags, n_keywords=K)
    B = binding.cooccur_matrix(tallied_of(cut_rows(counts, 7, N)), flags, n_keywords=K)
    check(A, a, "texts 0..6")
    check(B, b, "texts 7..13")
    check(binding.cooccur_add(A, B), want, ("the halves", flags))
    check(binding.cooccur_add(B, A), want, ("the halves, the other way round", flags))
    check(binding.cooccur_add(cooccurred_of(a), cooccurred_of(b)), add_expected(a, b), "the brute force agrees")
    # A over four keywords (the dictionary grew between the batches)
    first = cut_rows(counts, 0, 7)
    assert int(first[1].max()) < 4
    A4 = binding.cooccur_matrix(tallied_of(first), flags, n_keywords=4)
    assert A4.n_keywords == 4 and B.n_keywords == 5
    check(binding.cooccur_add(A4, B), want, ("4 keywords, then 5", flags))
    # three parts, either way, and a row_limit
    for limit in (0, 3):
        whole = brute_force(counts, K, flags, limit)
        parts = [binding.cooccur_matrix(tallied_of(cut_rows(counts, lo, hi)), flags, limit, K) for lo, hi in ((0, 3), (3, 9), (9, N))]
        check(binding.cooccur_add(binding.cooccur_add(parts[0], parts[1]), parts[2]), whole, "(a b) c")
        check(binding.cooccur_add(parts[0], binding.cooccur_add(parts[1], parts[2])), whole, "a (b c)")


def test_add_wraps_modulo_2_to_the_64():
    a = brute_force(matrix_of([{0: 1 << 63, 1: 3}]), 2, PRODUCT | DIAGONAL)
    b = brute_force(matrix_of([{0: (1 << 63) + 1, 1: 5}, {1: 1 << 32}]), 2, PRODUCT | DIAGONAL)
    want = add_expected(a, b)
    assert want.entries()[(0, 1)] == (3 * (1 << 63) + 5 * ((1 << 63) + 1)) & MASK and want.entries()[(1, 1)] == 34
    check(binding.cooccur_add(cooccurred_of(a), cooccurred_of(b)), want, "wrap")


def _add_raw(a, b, out_ptr, out_col, out_val, cap, n, n_a=None, n_b=None, a_ptr=None, b_ptr=None, a_col=None):
    def p(x):
        return x.ctypes.data if x is not None else None
    ap = a.co_ptr if a_ptr is None else a_ptr
    bp = b.co_ptr if b_ptr is None else b_ptr
    return acm.lib().acm_cooccur_add(p(ap), p(a.co_col if a_col is None else a_col), p(a.co_val), a.n_keywords if n_a is None else n_a, p(bp), p(b.co_col),
                                     p(b.co_val), b.n_keywords if n_b is None else n_b, p(out_ptr), p(out_col), p(out_val), cap,
                                     C.byref(n) if n is not None else None)


def test_add_arguments_overflow_and_count_only(counts):
    want = brute_force(counts, K, DIAGONAL)
    a, b = brute_force(cut_rows(counts, 0, 7), K, DIAGONAL), brute_force(cut_rows(counts, 7, N), K, DIAGONAL)
    k = want.nnz
    n = C.c_uint64(99)
    ptr, col, val = np.full(K + 1, GUARD64, np.uint64), np.full(k, GUARD32, np.uint32), np.full(k, GUARD64, np.uint64)
    assert _add_raw(a, b, ptr, None, None, 0, n) == 0 and n.value == k and np.array_equal(ptr, want.co_ptr)
    ptr[:] = GUARD64
    assert _add_raw(a, b, ptr, col, val, k - 1, n) == E_OVERFLOW
    assert n.value == k and np.array_equal(ptr, want.co_ptr) and np.all(col == GUARD32) and np.all(val == GUARD64)
    assert _add_raw(a, b, ptr, col, val, k, n) == 0 and np.array_equal(col, want.co_col) and np.array_equal(val, want.co_val)
    assert _add_raw(a, b, ptr, col, val, k, n, n_a=K, n_b=K - 1) == E_ARG              # n_keywords_a > n_keywords_b
    a4 = brute_force(cut_rows(counts, 0, 7), 4, DIAGONAL)
    assert _add_raw(b, a4, ptr, col, val, k, n) == E_ARG and _add_raw(a4, b, ptr, col, val, k, n) == 0
    down = a.co_ptr.copy()
    down[1], down[2] = a.co_ptr[2], a.co_ptr[1]
    assert down[1] > down[2] and _add_raw(a, b, ptr, col, val, k, n, a_ptr=down) == E_ARG
    one = b.co_ptr.copy()
    one[0] = 1
    assert _add_raw(a, b, ptr, col, val, k, n, b_ptr=one) == E_ARG
    high = a.co_col.copy()
    high[-1] = K
    assert _add_raw(a, b, ptr, col, val, k, n, a_col=high) == E_ARG                    # a col >= n_keywords_b
    assert _add_raw(a, b, None, col, val, k, n) == E_ARG and _add_raw(a, b, ptr, col, val, k, None) == E_ARG
    assert _add_raw(a, b, ptr, col, val, 1 << 31, n) == E_ARG and _add_raw(a, b, ptr, col, val, k, n, n_a=1 << 32, n_b=1 << 32) == E_ARG


def test_machine_cooccur_on_the_host_loop(counts):
    """3-byte symbols: no GPU path takes the machine.  "us|hers" and "sh|e" cut a keyword by a text boundary"""
    m = acm.Machine(3)                                                   # ACM_CMP_DEFAULT over 3 bytes: the host loop
    for kw in EXAMPLE_KEYWORDS:
        buf = np.frombuffer(sym3(kw), np.uint8).copy()
        m._keep.append(buf)
        cur = C.c_void_p(m.L.acm_initiate(m.handle))
        for i in range(len(kw)):
            m.L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + 3 * i)
        m.L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    texts = [sym3(t) for t in EXAMPLE_TEXTS]
    total = int(counts[2].sum())
    for flags in ALL_FLAGS:
        for limit in (0, 3):
            got = m.cooccur(texts, flags, limit)
            assert m.scan_path == PATH_LOOP and got.total == total
            check(got, brute_force(counts, K, flags, limit), ("Machine.cooccur", flags, limit))
    check(m.cooccur(texts, DIAGONAL, n_keywords=K + 2), brute_force(counts, K + 2, DIAGONAL), "Machine.cooccur, more keywords")
    # through the C call: one entry too little room is an overflow that leaves the entries alone; the path is recorded
    raw = np.frombuffer(b"".join(texts), np.uint8).copy()
    off = offsets_of(EXAMPLE_TEXTS)
    want = brute_force(counts, K)
    k = want.nnz
    ptr, col, val = np.zeros(K + 1, np.uint64), np.full(k - 1, GUARD32, np.uint32), np.full(k - 1, GUARD64, np.uint64)
    n, cross, skipped, tot = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)

    def call(n_keywords=K, flags=0, cap=k - 1):
        return m.L.acm_cooccur(m.handle, raw.ctypes.data, off.ctypes.data, off.size - 1, n_keywords, flags, 0, ptr.ctypes.data, col.ctypes.data,
                               val.ctypes.data, cap, C.byref(n), C.byref(cross), C.byref(skipped), C.byref(tot))
    assert call() == E_OVERFLOW and (n.value, cross.value, skipped.value, tot.value) == (k, want.cross, 0, total) and np.array_equal(ptr, want.co_ptr)
    assert np.all(col == GUARD32) and np.all(val == GUARD64)
    assert call(n_keywords=K - 1) == E_ARG and call(flags=4) == E_ARG and call(n_keywords=1 << 32) == E_ARG and call(cap=1 << 31) == E_ARG
    empty = m.cooccur([])
    assert (empty.nnz, empty.cross, empty.skipped) == (0, 0, 0) and empty.co_ptr.tolist() == [0] * (K + 1)


def test_plan_level_calls_refuse_a_missing_plan_before_they_touch_a_device():
    L = acm.lib()
    n = C.c_uint64(0)
    off = np.zeros(1, np.uint64)
    assert L.acm_gpu_cooccur_matrix_tmp_bytes(None, 0, 0, 0) == 0 and L.acm_gpu_cooccur_add_tmp_bytes(None, 0, 0) == 0
    assert L.acm_gpu_cooccur_tmp_bytes(None, 16, 16, 16, 0, 0, 0, 0) == 0
    assert L.acm_gpu_cooccur_matrix_device(None, None, None, None, 0, 0, 0, 0, 0, None, None, None, 0, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_cooccur_add_device(None, None, None, None, 0, None, None, None, 0, 0, None, None, None, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_cooccur_device(None, None, 0, None, 0, 16, 16, 16, 0, 0, 0, 0, None, None, None, 0, None, None, None, None, None, None, None, 0,
                                    None) == E_ARG
    assert L.acm_gpu_cooccur_host(None, None, off.ctypes.data, 0, 0, 0, 0, off.ctypes.data, None, None, 0, C.byref(n), None, None, None) == E_ARG


def _header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)            # comments mention functions too
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M)


def _declared():
    return set(re.findall(r"\b(acm_[a-z0-9_]+)\s*\(", _header_text()))


def test_export_list_is_the_header_and_apart_from_the_other_lists():
    L = acm.lib()
    assert _declared() == set(binding.COOCCUR_EXPORTS) and len(binding.COOCCUR_EXPORTS) == 10
    assert not set(binding.COOCCUR_EXPORTS) & (set(binding.EXPORTS) | set(binding.NEAR_EXPORTS))
    for name in binding.COOCCUR_EXPORTS:
        assert getattr(L, name) is not None, name
    nm = subprocess.run(["nm", "-D", "--defined-only", acm.library_path()], capture_output=True, check=True).stdout.decode()
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    assert set(s for s in exported if "cooccur" in s and s.startswith("acm_")) == set(binding.COOCCUR_EXPORTS)
    whole = open(os.path.join(ROOT, "include", "acm_gpu.h")).read()
    assert '#include "acm_cooccur.h"' in whole.split("#endif")[-1]
    assert whole.split("#endif")[-1].index('"acm_near.h"') < whole.split("#endif")[-1].index('"acm_cooccur.h"')
    assert "acm_cooccur" not in re.sub(r"/\*.*?\*/", " ", whole, flags=re.S).replace('"acm_cooccur.h"', "")
    assert (acm.ACM_COOCCUR_PRODUCT, acm.ACM_COOCCUR_DIAGONAL) == (1, 2)
    assert re.search(r"#define ACM_COOCCUR_PRODUCT 1u\s", open(HEADER).read()) and re.search(r"#define ACM_COOCCUR_DIAGONAL 2u\s", open(HEADER).read())


def test_signatures_agree_with_the_header():
    L = acm.lib()
    found = {}
    for ret, name, params in PROTOTYPE.findall(_header_text()):
        params = [] if params.strip() in ("", "void") else [c_class(p) for p in params.split(",")]
        assert name not in found
        found[name] = (c_class(ret, is_return=True), params)
    assert set(found) == set(binding.COOCCUR_EXPORTS)
    assert {name: (proto, signature(L, name)) for name, proto in found.items() if signature(L, name) != proto} == {}


def test_header_compiles_as_c11_and_every_declared_function_links(tmp_path):
    """include/acm_cooccur.h on its own after acm_gpu.h, and first of all"""
    for k, head in enumerate(('#include "aho_corasick.h"\n#include "acm_gpu.h"\n#include "acm_cooccur.h"\n', '#include "acm_cooccur.h"\n')):
        src = tmp_path / ("link_check_%d.c" % k)
        src.write_text(head + "int main(void){" + "".join("(void)%s;" % n for n in sorted(_declared())) +
                       "return (int)(ACM_COOCCUR_PRODUCT | ACM_COOCCUR_DIAGONAL) - 3;}\n")
        exe = str(tmp_path / ("link_check_%d" % k))
        p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                            "-L", os.path.dirname(acm.library_path()), "-lac75_amd", "-Wl,-rpath," + os.path.dirname(acm.library_path())],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
