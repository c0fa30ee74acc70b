"""Unordered keyword proximity on the host (acm_near_check, acm_near_records, the host path of acm_scan_near,
the header and the binding's list).  The expected answer is always the definition of NEAR in plain Python
(tests/near_cases.py): every first symbol S tried downwards over the ORACLE's records and, for byte text, a
second derivation from the text alone -- never the library's own scan or join, and never its closed form.  All
comparisons are exact, order included.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.near_cases import (CASE_CUT, CASE_GROUPS, CASE_KEYWORDS, CASE_TEXT, brute, case_facts, near, near_by_text, near_groups, oracle_records,
                              random_cases)
from tests.tally_cases import loop_machine, sym3
from tests.test_binding_signatures import PROTOTYPE, c_class, signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "acm_near.h")
E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
PATH_LOOP = 3
WIDTH_MAX = 1 << 20


def _same(got, want, what=None):
    assert got.size == want.size and np.array_equal(np.asarray(got).astype(po.RECORD_DTYPE), want), (what, got.size, want.size, got[:8], want[:8])


def _check(group_list, n_keywords, terms=None, group_ptr=None, groups=None, n_groups=None):
    """acm_near_check on a list of groups, or on raw arrays"""
    ns = binding.NearSet(group_list)
    t = ns.terms if terms is None else np.asarray(terms, np.uint32)
    p = ns.group_ptr if group_ptr is None else np.asarray(group_ptr, np.uint64)
    g = ns.groups if groups is None else np.asarray(groups, np.uint32).reshape(-1, 2)
    n = ns.n_groups if n_groups is None else n_groups
    return acm.lib().acm_near_check(t.ctypes.data if t.size else None, p.ctypes.data, g.ctypes.data if g.size else None, n, n_keywords)


def test_near_check_names_every_argument_error():
    ok = [([0, 1], 40, 0), ([1], 3, 1)]
    assert _check(ok, 2) == 0
    assert _check([], 0) == 0                                                    # no group is a set
    assert _check(ok, 2, group_ptr=[0, 2, 2], n_groups=2) == E_ARG               # a group without terms
    assert _check([(list(range(16)), 9, 16)], 16) == 0                           # 16 terms, the most, and need = m
    assert _check([(list(range(17)), 9, 0)], 17) == E_ARG                        # 17 terms
    assert _check([([0, 1, 0], 9, 0)], 2) == E_ARG                               # the same keyword twice in one group
    assert _check([([0, 1], 9, 0), ([1, 0], 9, 0)], 2) == 0                      # (in two groups it may stand)
    assert _check(ok, 1) == E_ARG                                                # keyword_id >= n_keywords
    assert _check([([0], 0, 0)], 1) == E_ARG                                     # width 0
    assert _check([([0], WIDTH_MAX, 0)], 1) == 0                                 # width = 2^20: the widest
    assert _check([([0], WIDTH_MAX + 1, 0)], 1) == E_ARG                         # width > 2^20
    assert _check([([0, 1], 9, 2)], 2) == 0 and _check([([0, 1], 9, 3)], 2) == E_ARG   # need = m, need > m
    assert _check([([0], 9, 0)], 1, groups=[(9, 0), (0, 0)]) == 0                # (groups[] is read for n_groups entries only)
    assert _check(ok, 2, group_ptr=[0, 3, 2], n_groups=2) == E_ARG               # group_ptr decreases
    assert _check(ok, 2, group_ptr=[1, 2, 3], n_groups=2) == E_ARG               # group_ptr does not begin with 0
    assert _check(ok, 2, n_groups=1 << 31) == E_ARG                              # (checked before group_ptr is read that far)
    assert _check([([0], 9, 0)], 1, group_ptr=[0, 1 << 31], n_groups=1) == E_ARG  # 2^31 terms (checked before terms[] is read)
    assert acm.lib().acm_near_check(None, None, None, 0, 0) == E_ARG
    with pytest.raises(acm.ACMError):
        binding.NearSet(ok).check(1)
    binding.NearSet(ok).check(2)
    # the ways to write a group
    ns = binding.NearSet([[0, 1], ([1, 2], 7), ([2], 5, 1)], width=40)
    assert near_groups(ns) == [([0, 1], 40, 0), ([1, 2], 7, 0), ([2], 5, 1)] and ns.n_keywords == 3
    with pytest.raises(ValueError):
        binding.NearSet([[0, 1]])


def test_the_two_derivations_agree_on_the_fixed_case_and_the_case_is_not_trivial():
    rec = oracle_records(CASE_KEYWORDS, CASE_TEXT)
    for offsets in (None, [0, CASE_CUT, len(CASE_TEXT)]):
        _same(near(rec, CASE_GROUPS, len(CASE_TEXT), offsets), near_by_text(CASE_KEYWORDS, CASE_GROUPS, CASE_TEXT, offsets), offsets)
    per, ties, two, far, lost = case_facts(CASE_KEYWORDS, CASE_GROUPS, CASE_TEXT, CASE_CUT)
    print("records %d, matches per group %s, ties %d, ends with two anchors %d, of them with the window at the farther anchor %d, lost to the cut %d"
          % (rec.size, per, ties, two, far, lost))
    assert per[5] == 0 and min(per[:5] + per[6:]) >= 2                           # group 6 is narrower than its keyword: nothing
    assert ties >= 2 and two >= 1 and far >= 1 and lost >= 1


def test_near_records_on_the_fixed_case():
    text = CASE_TEXT
    rec = oracle_records(CASE_KEYWORDS, text)
    nk = len(CASE_KEYWORDS)
    want = near(rec, CASE_GROUPS, len(text))
    _same(binding.near_records(rec, CASE_GROUPS, len(text), n_keywords=nk), want)
    off = np.array([0, CASE_CUT, len(text)], np.uint64)
    _same(binding.near_records(rec, CASE_GROUPS, len(text), offsets=off, n_keywords=nk), near(rec, CASE_GROUPS, len(text), off))
    # count-only, overflow (nothing written), the exact room
    L = acm.lib()
    ns = binding.NearSet(CASE_GROUPS)
    n = C.c_uint64(0)

    def call(out, cap, records=rec, n_symbols=len(text), pos_base=0, off=None, n_texts=0):
        return L.acm_near_records(records.ctypes.data, records.size, n_symbols, pos_base, off.ctypes.data if off is not None else None, n_texts,
                                  *ns.args(), nk, out.ctypes.data if out is not None else None, cap, C.byref(n))
    assert call(None, 0) == 0 and n.value == want.size
    out = np.zeros(want.size, po.RECORD_DTYPE)
    out["end_pos"] = 0x5555
    n.value = 0
    assert call(out, want.size - 1) == E_OVERFLOW and n.value == want.size and np.all(out["end_pos"] == 0x5555)
    assert call(out, want.size) == 0 and n.value == want.size
    _same(out, want)
    # positions across 2^32 and with bit 63 set
    for base in ((1 << 32) - 20, (1 << 63) + 5):
        shifted, moved = rec.copy(), want.copy()
        shifted["end_pos"] += np.uint64(base)
        moved["end_pos"] += np.uint64(base)
        _same(near(shifted, CASE_GROUPS, len(text), pos_base=base), moved)
        _same(binding.near_records(shifted, CASE_GROUPS, len(text), pos_base=base, n_keywords=nk), moved, base)
        _same(binding.near_records(shifted, CASE_GROUPS, len(text), offsets=off, pos_base=base, n_keywords=nk),
              near(shifted, CASE_GROUPS, len(text), off, pos_base=base), base)
    # records outside [pos_base, pos_base + n_symbols), their end or their start, or of length 0; offsets that break the contract
    assert call(out, want.size, records=shifted) == E_ARG                        # ends behind the buffer
    assert call(out, want.size, n_symbols=int(rec["end_pos"][-1])) == E_ARG      # the last record ends at n_symbols
    assert call(out, want.size, pos_base=1) == E_ARG                             # the first record begins in front of pos_base
    zero = rec.copy()
    zero["length"][3] = 0
    assert call(out, want.size, records=zero) == E_ARG
    for bad in ([0, 10, 5, len(text)], [1, len(text)], [0, len(text) - 1]):
        assert call(out, want.size, off=np.array(bad, np.uint64), n_texts=len(bad) - 1) == E_ARG
    _same(out, want)                                                             # nothing was written by the refused calls


def test_near_records_equals_the_definition_and_the_text_on_300_random_cases():
    matches = ties = cut_trials = nonempty = 0
    for trial, (kws, group_list, text, offsets, rec, want) in enumerate(random_cases()):
        _same(want, near_by_text(kws, group_list, text, offsets), (trial, "the two derivations"))
        got = binding.near_records(rec, group_list, len(text), offsets=offsets, n_keywords=len(kws))
        _same(got, want, (trial, kws, group_list, text, offsets))
        if offsets.size == 2:                                                    # one text: offsets NULL says the same
            _same(binding.near_records(rec, group_list, len(text), n_keywords=len(kws)), want, trial)
        matches += want.size
        nonempty += want.size > 0
        ties += int(np.count_nonzero(want["end_pos"][1:] == want["end_pos"][:-1]))
        cut_trials += offsets.size > 2
    print("matches %d in %d of 300 cases, ties in end_pos %d, trials with cuts %d" % (matches, nonempty, ties, cut_trials))
    assert nonempty >= 150 and ties > 100 and cut_trials > 100


def test_width_boundaries_and_special_shapes():
    kws = [b"ab", b"bc", b"x", b"y", b"abc"]

    def run(text, group_list, offsets=None):
        rec = oracle_records(kws, text)
        want = near(rec, group_list, len(text), offsets)
        _same(want, near_by_text(kws, group_list, text, offsets), text)
        _same(binding.near_records(rec, group_list, len(text), offsets=offsets, n_keywords=len(kws)), want, text)
        return [tuple(int(v) for v in r) for r in want]
    # a cover of span exactly `width` is found, of span width + 1 it is not; either order
    assert run(b"x..y", [([2, 3], 4, 0)]) == [(3, 4, 0)] and run(b"x..y", [([2, 3], 3, 0)]) == []
    assert run(b"y..x", [([2, 3], 4, 0)]) == [(3, 4, 0)] and run(b"y..x", [([2, 3], 3, 0)]) == []
    assert run(b"xx.y.x", [([2, 3], 9, 0)]) == [(3, 3, 0), (5, 3, 0)]             # the shortest window per end
    assert run(b"abc", [([0, 1], 3, 0)]) == [(2, 3, 0)]                           # ab and bc overlap: NEAR takes them
    assert run(b"abc", [([0, 1, 4], 3, 0)]) == [(2, 3, 0)]                        # ... and the nested three: one record per end
    assert run(b"abc", [([0, 4], 3, 1)]) == [(1, 2, 0), (2, 3, 0)]                # need 1: every record of the group
    assert run(b"abc", [([4], 3, 0)]) == [(2, 3, 0)] and run(b"abc", [([4], 2, 0)]) == []   # one term: its records no longer than the width
    assert run(b"x.y", [([2, 3], WIDTH_MAX, 0)]) == [(2, 3, 0)]                   # the window's lower end clamps at the buffer's first symbol
    assert run(b"x.y", [([2, 3], 9, 0)], [0, 1, 3]) == [] and run(b"x.y", [([2, 3], 9, 0)], [0, 0, 3, 3]) == [(2, 3, 0)]   # a cut behind x
    assert run(b"xyxy", [([2, 3], 2, 0), ([3, 2], 2, 0)]) == [(1, 2, 0), (1, 2, 1), (2, 2, 0), (2, 2, 1), (3, 2, 0), (3, 2, 1)]   # ties: group id ascending
    # symbols wider than a byte
    words = [[70000, 70001], [5]]
    t4 = np.array([70000, 70001, 9, 9, 5, 70000, 70001, 5, 5], np.uint32)
    wide = [([1, 0], 5, 0)]
    rec4 = brute(words, t4)
    want = near(rec4, wide, t4.size)
    assert [tuple(int(v) for v in r) for r in want] == [(4, 5, 0), (6, 3, 0), (7, 3, 0), (8, 4, 0)]
    _same(binding.near_records(rec4, wide, t4.size, n_keywords=2), want)


def _scan_near(h, text, n_symbols, group_list, cap, offsets=None):
    L = acm.lib()
    ns = binding.NearSet(group_list)
    out = np.zeros(max(cap, 1), po.RECORD_DTYPE)
    n = C.c_uint64(0)
    off = np.ascontiguousarray(offsets, np.uint64) if offsets is not None else None
    buf = np.frombuffer(text, np.uint8)
    rc = L.acm_scan_near(h, buf.ctypes.data if buf.size else None, n_symbols, off.ctypes.data if off is not None else None,
                         off.size - 1 if off is not None else 0, *ns.args(), out.ctypes.data if cap else None, cap, C.byref(n))
    return rc, int(n.value), out


def test_acm_scan_near_on_the_host_loop():
    """a machine with a comparator of its own over 3-byte symbols (tests/tally_cases.py): no GPU path takes it"""
    L = acm.lib()
    text = CASE_TEXT
    want = near_by_text(CASE_KEYWORDS, CASE_GROUPS, text)
    _same(want, near(oracle_records(CASE_KEYWORDS, text), CASE_GROUPS, len(text)))
    h, keep = loop_machine(CASE_KEYWORDS)
    assert L.acm_scan_path(h) == 0
    rc, n, out = _scan_near(h, sym3(text), len(text), CASE_GROUPS, want.size)
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    _same(out[:n], want)
    # too little room: the count that suffices comes back, the repeat succeeds; no room at all only counts
    rc, n, out = _scan_near(h, sym3(text), len(text), CASE_GROUPS, want.size - 1)
    assert rc == E_OVERFLOW and n == want.size and L.acm_scan_path(h) == PATH_LOOP
    rc, n, out = _scan_near(h, sym3(text), len(text), CASE_GROUPS, 0)
    assert rc == 0 and n == want.size
    # a batch: the same buffer cut into texts, empty ones among them
    offsets = np.array([0, 0, 31, CASE_CUT, CASE_CUT, len(text)], np.uint64)
    cut = near_by_text(CASE_KEYWORDS, CASE_GROUPS, text, offsets)
    assert 0 < cut.size < want.size
    rc, n, out = _scan_near(h, sym3(text), len(text), CASE_GROUPS, want.size, offsets=offsets)
    assert rc == 0
    _same(out[:n], cut)
    rc, n, out = _scan_near(h, b"", 0, CASE_GROUPS, 4)
    assert (rc, n) == (0, 0)
    # argument errors on this path too
    assert _scan_near(h, sym3(text), len(text), [([len(CASE_KEYWORDS)], 9, 0)], want.size)[0] == E_ARG
    assert _scan_near(h, sym3(text), len(text), [([0, 1], 9, 3)], want.size)[0] == E_ARG
    assert _scan_near(h, sym3(text), len(text), CASE_GROUPS, want.size, offsets=[0, 7, 5, len(text)])[0] == E_ARG
    L.acm_release(h)


def test_plan_level_calls_refuse_a_missing_plan_before_they_touch_a_device():
    L = acm.lib()
    ns = binding.NearSet(CASE_GROUPS)
    made, n = C.c_void_p(), C.c_uint64(0)
    info = binding.NearInfo()
    assert L.acm_gpu_near_create(None, *ns.args(), C.byref(made)) == E_ARG and not made.value
    assert L.acm_gpu_near_info(None, C.byref(info)) == E_ARG
    assert L.acm_gpu_near_tmp_bytes(None, None, 16, 0) == 0 and L.acm_gpu_scan_near_tmp_bytes(None, None, 16, 16, 0) == 0
    assert L.acm_gpu_near_records_device(None, None, None, 0, None, 0, 0, None, 0, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_near_device(None, None, None, 0, 0, None, 0, 0, None, 0, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_near_host(None, None, 0, 0, None, 0, *ns.args(), None, 0, C.byref(n)) == E_ARG
    L.acm_gpu_near_destroy(None)


def _header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)            # comments mention functions too
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M)


def _declared():
    return set(re.findall(r"\b(acm_[a-z0-9_]+)\s*\(", _header_text()))


def test_export_list_is_the_header_and_apart_from_the_five_headers_list():
    L = acm.lib()
    assert _declared() == set(binding.NEAR_EXPORTS) and len(binding.NEAR_EXPORTS) == 11
    assert not set(binding.NEAR_EXPORTS) & set(binding.EXPORTS)
    for name in binding.NEAR_EXPORTS:
        assert getattr(L, name) is not None, name
    tail = open(os.path.join(ROOT, "include", "acm_gpu.h")).read().split("#endif")[-1]
    assert '#include "acm_near.h"' in tail
    assert "acm_near" not in re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "acm_gpu.h")).read(), flags=re.S).replace('"acm_near.h"', "")


def test_signatures_agree_with_the_header():
    L = acm.lib()
    found = {}
    for ret, name, params in PROTOTYPE.findall(_header_text()):
        params = [] if params.strip() in ("", "void") else [c_class(p) for p in params.split(",")]
        assert name not in found
        found[name] = (c_class(ret, is_return=True), params)
    assert set(found) == set(binding.NEAR_EXPORTS)
    assert {name: (proto, signature(L, name)) for name, proto in found.items() if signature(L, name) != proto} == {}


def test_header_compiles_as_c11_and_every_declared_function_links(tmp_path):
    """include/acm_near.h on its own after acm_gpu.h, and first of all"""
    for k, head in enumerate(('#include "aho_corasick.h"\n#include "acm_gpu.h"\n#include "acm_near.h"\n', '#include "acm_near.h"\n')):
        src = tmp_path / ("link_check_%d.c" % k)
        src.write_text(head + "int main(void){" + "".join("(void)%s;" % n for n in sorted(_declared())) + "return 0;}\n")
        exe = str(tmp_path / ("link_check_%d" % k))
        p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                            "-L", os.path.dirname(acm.library_path()), "-lac75_amd", "-Wl,-rpath," + os.path.dirname(acm.library_path())],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
