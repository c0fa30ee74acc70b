"""The minimum-cost tiling without a GPU: acm_segment_records (the sequential pass on the host) and
acm_segment on a machine that takes the caller loop on the host (ACM_SCAN_PATH_CPU_LOOP).  The expected
answer is the definition of SEGMENT in plain Python over the ORACLE's records (tests/segment_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.batch_cases import KEYWORDS, TEXTS
from tests.segment_cases import EXAMPLES, define, example, exhaustive_minimum, random_cases
from tests.select_cases import assert_tiling, greedy, oracle_records
from tests.tally_cases import PATH_LOOP, byte_oracle, loop_machine, novel_words, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "acm_segment.h")
NAMES = ("acm_segment_records", "acm_gpu_segment_tmp_bytes", "acm_gpu_segment_records_device", "acm_gpu_scan_segment_tmp_bytes",
         "acm_gpu_scan_segment_device", "acm_gpu_scan_segment_host", "acm_segment")


def _same(got, want):
    assert got.size == want.size and np.array_equal(got.astype(po.RECORD_DTYPE), want), (got[:8], want[:8])


def test_worked_examples_of_the_header():
    for k in range(len(EXAMPLES)):
        rec, cost, gap, want, total, text, _ = example(k)
        by_rule, best = define(rec, cost, gap, 0, len(text))
        _same(by_rule, want)                                    # the table of the header is the definition's answer
        assert best == total
        got, sums = binding.segment_records(rec, cost, gap)
        _same(got, want)
        assert_tiling(got)
        assert sums[0] + gap * (len(text) - sums[1]) == total
    rec = example(1)[0]
    assert [(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in greedy(rec)] == [(2, 3, 1)]   # SELECT strands `d`
    rec = example(2)[0]
    assert int(greedy(rec)[-1]["length"]) == 1                  # SELECT puts the single `a` at the end


def test_random_cases_against_the_definition_and_the_exhaustive_minimum():
    differ = small = 0
    for keywords, text, cost, gap in random_cases():
        rec = oracle_records(byte_oracle(keywords), text)
        want, best = define(rec, cost, gap, 0, len(text))
        got, sums = binding.segment_records(rec, cost, gap)
        _same(got, want)
        assert sums == (int(sum(int(cost[k]) for k in want["keyword_id"])), int(want["length"].sum()))
        assert sums[0] + gap * (len(text) - sums[1]) == best
        g = greedy(rec)
        differ += want.size > 0 and not (want.size == g.size and np.array_equal(want, g))
        if rec.size <= 14:
            small += 1
            assert exhaustive_minimum(rec, cost, gap, len(text)) == best
    print("differ from SELECT: %d of 200; checked exhaustively: %d" % (differ, small))
    assert differ >= 100 and small >= 5


def test_the_result_does_not_depend_on_pos_lo_or_n():
    shift = 1 << 33
    for k, (keywords, text, cost, gap) in enumerate(random_cases(seed=7, count=30)):
        rec = oracle_records(byte_oracle(keywords), text)
        want, _ = define(rec, cost, gap)
        _same(define(rec, cost, gap, -5, len(text) + 40)[0], want)
        moved = rec.copy()
        moved["end_pos"] += shift
        got, _ = binding.segment_records(moved, cost, gap)
        got["end_pos"] -= shift
        _same(got, want)


def test_in_place_empty_and_single_record_sets():
    L = acm.lib()
    rec, cost, gap, want, _, _, _ = example(1)
    buf = rec.copy()
    n = C.c_uint64(99)
    sums = np.zeros(2, np.uint64)
    assert L.acm_segment_records(buf.ctypes.data, buf.size, cost.ctypes.data, cost.size, gap, C.byref(n), sums.ctypes.data) == 0
    _same(buf[:n.value], want)                                  # in the front of the input array itself
    buf = rec.copy()
    assert L.acm_segment_records(buf.ctypes.data, rec.size, cost.ctypes.data, cost.size, gap, C.byref(n), None) == 0   # sums may be NULL
    _same(buf[:n.value], want)
    got, sums = binding.segment_records(np.zeros(0, po.RECORD_DTYPE), cost, gap)
    assert got.size == 0 and sums == (0, 0)
    n = C.c_uint64(99)
    assert L.acm_segment_records(None, 0, None, 0, 0, C.byref(n), None) == 0 and n.value == 0
    one = np.array([(7, 3, 2)], po.RECORD_DTYPE)
    got, sums = binding.segment_records(one, [9, 9, 4], 2)      # 4 <= 3 * 2: the keyword is taken
    _same(got, one)
    assert sums == (4, 3)
    got, sums = binding.segment_records(one, [9, 9, 7], 2)      # 7 > 6: the symbols stay uncovered
    assert got.size == 0 and sums == (0, 0)
    got, _ = binding.segment_records(one, [9, 9, 6], 2)         # a tie: the keyword wins
    _same(got, one)


def test_arguments_are_checked_and_nothing_is_modified():
    L = acm.lib()
    rec, cost, gap, _, _, _, _ = example(0)
    n = C.c_uint64(0)

    def call(records=rec, cost=cost, n_keywords=None, gap=gap, count=C.byref(n)):
        buf = records.copy()
        rc = L.acm_segment_records(buf.ctypes.data, buf.size, cost.ctypes.data if cost is not None else None,
                                   cost.size if n_keywords is None else n_keywords, gap, count, None)
        assert rc == 0 or np.array_equal(buf, records)
        return rc
    assert call() == 0
    big = cost.copy()
    big[0] = 1 << 24
    assert call(cost=big) == E_ARG and call(gap=1 << 24) == E_ARG
    big[0] = (1 << 24) - 1
    assert call(cost=big) == 0 and call(gap=(1 << 24) - 1) == 0
    assert call(n_keywords=3) == E_ARG                          # `hers` is keyword 3
    assert call(cost=None, n_keywords=4) == E_ARG and call(count=None) == E_ARG
    assert L.acm_segment_records(None, 3, cost.ctypes.data, 4, gap, C.byref(n), None) == E_ARG
    bad = rec.copy()
    bad["length"][1] = 0
    assert call(records=bad) == E_ARG
    assert call(records=rec[::-1].copy()) == E_ARG              # ends that descend


def _segment(h, text3, cost, gap, capacity):
    L = acm.lib()
    t = np.frombuffer(text3, np.uint8).copy() if len(text3) else np.zeros(3, np.uint8)
    out = np.zeros(max(capacity, 1), po.RECORD_DTYPE)
    n = C.c_uint64(0xDEAD)
    sums = np.zeros(2, np.uint64)
    rc = L.acm_segment(h, t.ctypes.data, len(text3) // 3, cost.ctypes.data, cost.size, gap, out.ctypes.data, capacity, C.byref(n), sums.ctypes.data)
    return rc, int(n.value), out, sums


def test_acm_segment_on_the_host_loop(novel_bytes):
    L = acm.lib()
    for keywords, text in ((KEYWORDS + [b"absent"], b"".join(TEXTS)), (novel_words(novel_bytes), novel_bytes[:60000])):
        rec = oracle_records(byte_oracle(keywords), text)
        cost = (1 + np.arange(len(keywords)) % 5).astype(np.uint32)
        want, best = define(rec, cost, 8, 0, len(text))
        assert 0 < want.size < rec.size
        h, keep = loop_machine(keywords)
        assert L.acm_scan_path(h) == 0
        rc, n, out, sums = _segment(h, sym3(text), cost, 8, rec.size)
        assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
        _same(out[:n], want)
        assert int(sums[0]) + 8 * (len(text) - int(sums[1])) == best
        # too little room for ALL matches: the count that suffices comes back, the repeat succeeds
        rc, n, out, _ = _segment(h, sym3(text), cost, 8, rec.size - 1)
        assert rc == E_OVERFLOW and n == rec.size
        rc, n, out, _ = _segment(h, sym3(text), cost, 8, n)
        assert rc == 0
        _same(out[:n], want)
        rc, n, out, sums = _segment(h, b"", cost, 8, 4)
        assert (rc, n, int(sums[0]), int(sums[1])) == (0, 0, 0, 0)
        assert _segment(h, sym3(text), cost[:-1], 8, rec.size)[0] == E_ARG      # a table that does not cover the machine's keywords
        big = cost.copy()
        big[-1] = 1 << 24
        assert _segment(h, sym3(text), big, 8, rec.size)[0] == E_ARG
        L.acm_release(h)


def test_segment_arguments_are_checked_without_a_gpu():
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    t = np.zeros(3, np.uint8)
    out = np.zeros(4, po.RECORD_DTYPE)
    cost = np.ones(len(KEYWORDS), np.uint32)
    n = C.c_uint64(0)
    args = (cost.ctypes.data, cost.size, 1)
    assert L.acm_segment(None, t.ctypes.data, 1, *args, out.ctypes.data, 4, C.byref(n), None) == E_ARG
    assert L.acm_segment(h, None, 1, *args, out.ctypes.data, 4, C.byref(n), None) == E_ARG
    assert L.acm_segment(h, t.ctypes.data, 1, *args, None, 4, C.byref(n), None) == E_ARG
    assert L.acm_segment(h, t.ctypes.data, 1, *args, out.ctypes.data, 4, None, None) == E_ARG
    assert L.acm_segment(h, t.ctypes.data, 1, None, cost.size, 1, out.ctypes.data, 4, C.byref(n), None) == E_ARG
    assert L.acm_segment(h, t.ctypes.data, 1, cost.ctypes.data, cost.size, 1 << 24, out.ctypes.data, 4, C.byref(n), None) == E_ARG
    assert L.acm_scan_path(h) == 0
    # the plan-level calls refuse a missing plan before they touch a device
    assert L.acm_gpu_segment_records_device(None, None, 0, None, 0, 0, cost.ctypes.data, cost.size, 1, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_segment_device(None, None, 0, 0, None, 0, cost.ctypes.data, cost.size, 1, None, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_segment_host(None, t.ctypes.data, 1, 0, None, 0, cost.ctypes.data, cost.size, 1, out.ctypes.data, 4, C.byref(n), None) == E_ARG
    assert L.acm_gpu_segment_tmp_bytes(None, 16, 16) == 0 and L.acm_gpu_scan_segment_tmp_bytes(None, 16, 16, 0) == 0
    L.acm_release(h)


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)                # comments mention functions too
    return set(re.findall(r"\b(acm_[a-z0-9_]+)\s*\(", text))


def test_library_exports_the_segment_symbols():
    L = acm.lib()
    for name in NAMES:
        assert name in binding.EXPORTS and getattr(L, name) is not None, name


def test_export_list_covers_the_header():
    assert _declared() == set(NAMES) and _declared() <= set(binding.EXPORTS)
    assert open(os.path.join(ROOT, "include", "acm_gpu.h")).read().rstrip().endswith('#include "acm_segment.h"')


def test_header_compiles_as_c11_and_every_declared_function_links(tmp_path):
    """include/acm_segment.h on its own after acm_gpu.h, and first of all"""
    for k, head in enumerate(('#include "aho_corasick.h"\n#include "acm_gpu.h"\n#include "acm_segment.h"\n', '#include "acm_segment.h"\n')):
        src = tmp_path / ("link_check_%d.c" % k)
        src.write_text(head + "int main(void){" + "".join("(void)%s;" % n for n in sorted(_declared())) + "return 0;}\n")
        exe = str(tmp_path / ("link_check_%d" % k))
        pkg = os.path.join(ROOT, "aho-corasick-1975_amd")
        p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                            "-L", pkg, "-lac75_amd", "-Wl,-rpath," + pkg],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
