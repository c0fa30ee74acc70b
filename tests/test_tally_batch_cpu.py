"""Per-text keyword counts of a batch without a GPU: acm_tally_batch_records (the sequential pass) and
acm_tally_batch on a machine with a comparator of its own over 3-byte symbols, which takes the caller
loop on the host (ACM_SCAN_PATH_CPU_LOOP).  The expected answer is always derived from the ORACLE's
scan of every text alone (tests/tally_batch_cases.py)."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, offsets_of, oracle_batch_cut
from tests.grep_cases import GREP_TEXTS
from tests.tally_batch_cases import check, expected, nontrivial
from tests.tally_cases import PATH_LOOP, byte_oracle, loop_machine, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def _case():
    o = byte_oracle(KEYWORDS)
    text = np.frombuffer(b"".join(GREP_TEXTS), np.uint8)
    off = offsets_of(GREP_TEXTS)
    want = expected(o, text, off)
    nontrivial(o, text, off, want)
    return o, text, off, want


def test_records_on_the_boundary_cases():
    o, text, off, want = _case()
    rec, tid, first = oracle_batch_cut(o, text, off)
    check(binding.tally_batch_records(rec, first, len(KEYWORDS)), want, "records")
    # the records of every text in another order: the matrix is the same
    rng = np.random.default_rng(3)
    shuffled = rec.copy()
    for t in range(first.size - 1):
        a, b = int(first[t]), int(first[t + 1])
        shuffled[a:b] = rec[a:b][rng.permutation(b - a)]
    check(binding.tally_batch_records(shuffled, first, len(KEYWORDS) + 5), want, "records, shuffled")


def test_records_overflow_by_one_entry_and_count_only():
    o, text, off, want = _case()
    rec, tid, first = oracle_batch_cut(o, text, off)
    L = acm.lib()
    n, nnz = first.size - 1, want[1].size
    row_ptr = np.full(n + 1, GUARD64, np.uint64)
    col, val = np.full(nnz - 1, GUARD32, np.uint32), np.full(nnz - 1, GUARD64, np.uint64)
    need = C.c_uint64(99)
    rc = L.acm_tally_batch_records(rec.ctypes.data, first.ctypes.data, n, len(KEYWORDS), row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data,
                                   nnz - 1, C.byref(need))
    assert rc == E_OVERFLOW and need.value == nnz
    assert np.all(col == GUARD32) and np.all(val == GUARD64) and np.array_equal(row_ptr, want[0])
    # col and val NULL: the call only counts
    row_ptr[:] = GUARD64
    need.value = 99
    assert L.acm_tally_batch_records(rec.ctypes.data, first.ctypes.data, n, len(KEYWORDS), row_ptr.ctypes.data, None, None, 0, C.byref(need)) == 0
    assert need.value == nnz and np.array_equal(row_ptr, want[0])
    # exactly the room: guard entries behind it stay
    col, val = np.full(nnz + 3, GUARD32, np.uint32), np.full(nnz + 3, GUARD64, np.uint64)
    assert L.acm_tally_batch_records(rec.ctypes.data, first.ctypes.data, n, len(KEYWORDS), row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data,
                                     nnz, C.byref(need)) == 0
    assert np.array_equal(col[:nnz], want[1]) and np.array_equal(val[:nnz], want[2])
    assert np.all(col[nnz:] == GUARD32) and np.all(val[nnz:] == GUARD64)


def test_records_arguments_and_no_text():
    o, text, off, want = _case()
    rec, tid, first = oracle_batch_cut(o, text, off)
    L = acm.lib()
    n = first.size - 1
    row_ptr = np.zeros(n + 1, np.uint64)
    col, val = np.zeros(want[1].size, np.uint32), np.zeros(want[1].size, np.uint64)
    nnz = C.c_uint64(99)

    def call(f=first, n_texts=n, n_keywords=len(KEYWORDS), rp=row_ptr.ctypes.data, out=C.byref(nnz)):
        return L.acm_tally_batch_records(rec.ctypes.data, f.ctypes.data if f is not None else None, n_texts, n_keywords, rp, col.ctypes.data,
                                         val.ctypes.data, col.size, out)
    assert call() == 0
    down = first.copy()
    down[3], down[4] = first[4] + 1, first[3]
    assert down[3] > down[4] and call(f=down) == E_ARG
    one = first.copy()
    one[0] = 1
    assert call(f=one) == E_ARG
    assert int(rec["keyword_id"].max()) == 3 and call(n_keywords=3) == E_ARG                 # a keyword id >= n_keywords
    assert call(n_texts=1 << 31) == E_ARG and call(f=None) == E_ARG and call(rp=None) == E_ARG and call(out=None) == E_ARG
    # no text at all
    rp = np.full(1, 77, np.uint64)
    assert L.acm_tally_batch_records(None, np.zeros(1, np.uint64).ctypes.data, 0, 4, rp.ctypes.data, None, None, 0, C.byref(nnz)) == 0
    assert rp[0] == 0 and nnz.value == 0
    got = binding.tally_batch_records(np.zeros(0, po.RECORD_DTYPE), np.zeros(1, np.uint64), 4)
    assert got.nnz == 0 and got.total == 0 and got.row_ptr.tolist() == [0]
    # texts without any record
    got = binding.tally_batch_records(np.zeros(0, po.RECORD_DTYPE), np.zeros(4, np.uint64), 4)
    assert got.nnz == 0 and got.row_ptr.tolist() == [0, 0, 0, 0]


def test_tally_batch_on_the_host_loop():
    """3-byte symbols: no GPU path takes the machine.  "us|hers" and "sh|e" cut a keyword by a text boundary"""
    o, text, off, want = _case()
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    assert L.acm_scan_path(h) == 0
    raw = np.frombuffer(sym3(bytes(text)), np.uint8).copy()
    n, k = off.size - 1, want[1].size
    row_ptr = np.zeros(n + 1, np.uint64)
    col, val = np.full(k + 2, GUARD32, np.uint32), np.full(k + 2, GUARD64, np.uint64)
    nnz, total = C.c_uint64(99), C.c_uint64(99)
    rc = L.acm_tally_batch(h, raw.ctypes.data, off.ctypes.data, n, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, k, C.byref(nnz),
                           C.byref(total))
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    check(binding.TalliedBatch(row_ptr, col[:nnz.value], val[:nnz.value], int(nnz.value), int(total.value)), want, "acm_tally_batch")
    assert np.all(col[k:] == GUARD32) and np.all(val[k:] == GUARD64)
    # one entry too little room: the need, row_ptr and total valid, col and val untouched
    col[:], val[:], row_ptr[:] = GUARD32, GUARD64, 0
    nnz.value = total.value = 99
    rc = L.acm_tally_batch(h, raw.ctypes.data, off.ctypes.data, n, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, k - 1, C.byref(nnz),
                           C.byref(total))
    assert rc == E_OVERFLOW and nnz.value == k and total.value == int(want[2].sum()) and np.array_equal(row_ptr, want[0])
    assert np.all(col == GUARD32) and np.all(val == GUARD64)
    # col and val NULL: counting only; total is optional
    assert L.acm_tally_batch(h, raw.ctypes.data, off.ctypes.data, n, row_ptr.ctypes.data, None, None, 0, C.byref(nnz), None) == 0 and nnz.value == k
    # arguments: no machine, no row_ptr, no nnz, offsets that decrease
    bad = off.copy()
    bad[3], bad[4] = off[4] + 1, off[3]
    for args in ((None, off, row_ptr.ctypes.data, C.byref(nnz)), (h, off, None, C.byref(nnz)), (h, off, row_ptr.ctypes.data, None),
                 (h, bad, row_ptr.ctypes.data, C.byref(nnz))):
        assert L.acm_tally_batch(args[0], raw.ctypes.data, args[1].ctypes.data, n, args[2], None, None, 0, args[3], None) == E_ARG
    L.acm_release(h)


def test_tally_batch_on_the_host_loop_regrows_its_record_room():
    """one text of 3,000 x "s" between two short ones: more records than the 1,024 the loop starts with"""
    o = byte_oracle(KEYWORDS)
    texts = [b"ushers", b"s" * 3000, b"she"]
    text = np.frombuffer(b"".join(texts), np.uint8)
    off = offsets_of(texts)
    want = expected(o, text, off)
    assert int(want[2].sum()) > 1024 > text.size // 64
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    raw = np.frombuffer(sym3(bytes(text)), np.uint8).copy()
    n, k = off.size - 1, want[1].size
    row_ptr = np.zeros(n + 1, np.uint64)
    col, val = np.full(k + 2, GUARD32, np.uint32), np.full(k + 2, GUARD64, np.uint64)
    nnz, total = C.c_uint64(99), C.c_uint64(99)
    rc = L.acm_tally_batch(h, raw.ctypes.data, off.ctypes.data, n, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, k, C.byref(nnz),
                           C.byref(total))
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    check(binding.TalliedBatch(row_ptr, col[:nnz.value], val[:nnz.value], int(nnz.value), int(total.value)), want, "acm_tally_batch, regrown")
    assert np.all(col[k:] == GUARD32) and np.all(val[k:] == GUARD64)
    L.acm_release(h)


def test_plan_level_calls_refuse_before_they_touch_a_device():
    L = acm.lib()
    nnz = C.c_uint64(0)
    off = np.zeros(1, np.uint64)
    assert L.acm_gpu_tally_batch_tmp_bytes(None, 16, 16, 16, 0, 0) == 0
    assert L.acm_gpu_tally_batch_host(None, None, off.ctypes.data, 0, off.ctypes.data, None, None, 0, C.byref(nnz), None) == E_ARG
    assert L.acm_gpu_tally_batch_device(None, None, 0, None, 0, 16, 16, 16, None, None, None, None, None, None, None, None, 0, None) == E_ARG


def test_library_exports_the_tally_batch_symbols():
    L = acm.lib()
    for name in ("acm_tally_batch_records", "acm_gpu_tally_batch_tmp_bytes", "acm_gpu_tally_batch_device", "acm_gpu_tally_batch_host",
                 "acm_tally_batch"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
