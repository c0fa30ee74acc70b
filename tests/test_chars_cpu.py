"""Positions in code points and UTF-16 units without a GPU: acm_chars_positions and acm_chars_records (the sequential
definition) against the numpy definition of tests/chars_cases.py and against bytes.decode, acm_scan_chars and
Machine.scan_str on a machine that takes the caller loop on the host (ACM_SCAN_PATH_CPU_LOOP), the header and the
binding's list."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests import chars_cases as cc
from tests.tally_cases import PATH_LOOP
from tests.test_binding_signatures import PROTOTYPE, c_class, signature

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "acm_chars.h")
UNIT_NAMES = {cc.CODEPOINTS: "codepoints", cc.UTF16: "utf16"}


def test_the_worked_example_of_the_header():
    """the oracle's records of the example are the table's, and the table is the definition, bytes.decode and the C call"""
    o = cc.oracle_of(cc.EXAMPLE_KEYWORDS)
    text = np.frombuffer(cc.EXAMPLE_TEXT, np.uint8)
    assert text.tobytes().hex(" ") == "61 c3 a9 e2 82 ac f0 9f 98 80 20 c3 a9 f0 9f 98 80 61"
    rec = o.scan(text)
    assert [tuple(int(x) for x in r) for r in rec] == [row[0] for row in cc.EXAMPLE]
    for unit, col in ((cc.CODEPOINTS, 1), (cc.UTF16, 2)):
        start, length, edge = binding.chars_records(cc.EXAMPLE_TEXT, rec, unit=unit)
        assert [(int(a), int(b)) for a, b in zip(start, length)] == [row[col] for row in cc.EXAMPLE]
        assert edge.tolist() == [row[3] for row in cc.EXAMPLE]
        want = cc.records_expected(text, rec, unit=unit)
        assert np.array_equal(start, want[0]) and np.array_equal(length, want[1]) and np.array_equal(edge, want[2])
        whole = binding.chars_positions(cc.EXAMPLE_TEXT, [len(cc.EXAMPLE_TEXT)], unit=unit)
        assert int(whole[0]) == cc.EXAMPLE_TOTALS[col - 1]
    assert len(cc.EXAMPLE_STR) == 8 and len(cc.EXAMPLE_STR.encode("utf-16-le")) // 2 == 10


def _round_trips(text, rec, keywords):
    """every record with edge 0 on valid text is its keyword in the decoded string, in both units"""
    s = bytes(text).decode("utf-8")
    u16 = s.encode("utf-16-le")
    seen = 0
    for unit in cc.UNITS:
        start, length, edge = binding.chars_records(text, rec, unit=unit)
        for r, a, n, e in zip(rec, start, length, edge):
            kw = bytes(keywords[int(r["keyword_id"])])
            if e:
                continue
            seen += 1
            a, n = int(a), int(n)
            got = s[a:a + n] if unit == cc.CODEPOINTS else u16[2 * a:2 * (a + n)].decode("utf-16-le")
            assert got.encode("utf-8") == kw, (unit, r, a, n)
    return seen


def test_aligned_records_round_trip_through_decode():
    o = cc.oracle_of()
    for seed in (1, 2, 3):
        text = cc.valid_text(seed, 3000)
        rec = o.scan(np.frombuffer(text, np.uint8))
        edge = binding.chars_records(text, rec)[2]
        assert rec.size > 100 and np.any(edge == 0) and np.any(edge == 1) and np.any(edge == 2) and np.any(edge == 3)
        assert _round_trips(text, rec, cc.KEYWORDS) > 100


def _texts_with_cuts(seed, kind):
    """a buffer of the kind and offsets with empty texts first, last and adjacent and cuts anywhere (inside characters too)"""
    n = 2000
    text = cc.TEXT_KINDS[kind](seed, n)
    rng = np.random.default_rng(seed + 7)
    cuts = np.sort(rng.integers(0, n + 1, size=40)).astype(np.uint64)
    off = np.concatenate([[0, 0], cuts, cuts[10:12], [n, n, n]]).astype(np.uint64)
    off.sort()
    return text, off


@pytest.mark.parametrize("kind", list(cc.TEXT_KINDS))
@pytest.mark.parametrize("unit", cc.UNITS)
def test_host_definitions_against_numpy(kind, unit):
    o = cc.oracle_of()
    for seed in (11, 12):
        text, off = _texts_with_cuts(seed, kind)
        t = np.frombuffer(text, np.uint8)
        if kind in ("valid", "invalid"):
            assert any((t[int(a)] & 0xC0) == 0x80 for a in off[:-1] if a < t.size), "no text begins with a continuation byte"
        rec = o.scan(t)
        rng = np.random.default_rng(seed)
        rec = rec[rng.permutation(rec.size)]                              # any order
        if kind != "ascii":
            assert rec.size > 0
        pos = np.concatenate([np.arange(t.size + 1), off]).astype(np.uint64)
        for offsets in (None, off):
            got = binding.chars_positions(text, pos, offsets, unit)
            assert np.array_equal(got, cc.positions_expected(t, pos, offsets, unit)), (kind, unit, seed)
            for base in (0, (1 << 63) + 9):
                moved = rec.copy()
                moved["end_pos"] += np.uint64(base)
                got = binding.chars_records(text, moved, offsets, unit, pos_base=base)
                want = cc.records_expected(t, moved, offsets, unit, pos_base=base)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (kind, unit, seed, base)
        # the positions of a batch count from their text: a text's first position is 0
        assert np.all(binding.chars_positions(text, off[:-1], off, unit)[off[:-1] < t.size] == 0)
    # no text at all, and a buffer without a byte
    assert binding.chars_positions(b"", [0], None, unit).tolist() == [0]
    assert binding.chars_positions(b"", [0], np.zeros(1, np.uint64), unit).tolist() == [0]
    assert binding.chars_positions(b"", [0, 0], np.zeros(3, np.uint64), unit).tolist() == [0, 0]


def test_a_record_across_a_cut_counts_through_it_and_is_judged_by_the_byte_behind():
    text = "é€é".encode()                                                   # c3 a9 | e2 82 ac c3 a9, cut at 2 and inside the euro sign
    off = np.array([0, 2, 4, 7], np.uint64)
    rec = cc.rec_array([(4, 5, 0), (2, 1, 0), (3, 2, 0), (6, 4, 0)])
    start, length, edge = binding.chars_records(text, rec, off)
    # through the cut at 2; ending inside the euro sign; ending at the cut at 4; from inside the euro sign (the second byte of the text
    # that begins at 2) through the cut at 4 to the end of the buffer
    assert start.tolist() == [0, 0, 0, 1] and length.tolist() == [2, 1, 1, 1] and edge.tolist() == [0, 2, 0, 1]
    want = cc.records_expected(text, rec, off)
    assert np.array_equal(start, want[0]) and np.array_equal(length, want[1]) and np.array_equal(edge, want[2])


def _raw_records(text, rec, off=None, n_texts=0, unit=1, base=0, outs=(True, True, True), n_symbols=None, n=None):
    t = np.frombuffer(bytes(text), np.uint8)
    k = rec.size if n is None else n
    start, length, edge = np.full(max(k, 1), 0xA5, np.uint64), np.full(max(k, 1), 0xA5, np.uint32), np.full(max(k, 1), 0xA5, np.uint8)
    rc = acm.lib().acm_chars_records(t.ctypes.data if t.size else None, t.size if n_symbols is None else n_symbols, base,
                                     off.ctypes.data if off is not None else None, n_texts, unit, rec.ctypes.data if rec.size else None, k,
                                     start.ctypes.data if outs[0] else None, length.ctypes.data if outs[1] else None,
                                     edge.ctypes.data if outs[2] else None)
    untouched = bool(np.all(start == 0xA5) and np.all(length == 0xA5) and np.all(edge == 0xA5))
    return rc, untouched


def test_every_argument_error_leaves_the_outputs_alone():
    text = cc.EXAMPLE_TEXT
    n = len(text)
    rec = cc.rec_array([row[0] for row in cc.EXAMPLE])
    assert _raw_records(text, rec) == (0, False)
    assert _raw_records(text, rec, unit=0) == (E_ARG, True) and _raw_records(text, rec, unit=3) == (E_ARG, True)
    assert _raw_records(text, rec, outs=(False, False, False)) == (E_ARG, True)
    for outs in ((True, False, False), (False, True, False), (False, False, True)):
        assert _raw_records(text, rec, outs=outs)[0] == 0
    for bad_off in ([1, n], [0, n - 1], [0, 9, 8, n]):
        off = np.array(bad_off, np.uint64)
        assert _raw_records(text, rec, off, off.size - 1) == (E_ARG, True), bad_off
    good = np.array([0, 3, 3, n], np.uint64)
    assert _raw_records(text, rec, good, 3)[0] == 0
    for triple in ((n, 1, 0), (5, 0, 0), (3, 5, 0)):                         # behind the buffer, of length 0, a start below pos_base
        bad = np.concatenate([rec, cc.rec_array([triple])])
        assert _raw_records(text, bad) == (E_ARG, True), triple
    assert _raw_records(text, rec, base=1) == (E_ARG, True)                  # (the first record ends at 0: in front of pos_base)
    moved = rec.copy()
    moved["end_pos"] += np.uint64(100)
    assert _raw_records(text, moved, base=100)[0] == 0 and _raw_records(text, moved, base=101) == (E_ARG, True)
    # positions
    L = acm.lib()
    t = np.frombuffer(text, np.uint8)
    pos, out = np.array([0, n, n + 1], np.uint64), np.full(3, 0xA5, np.uint64)
    assert L.acm_chars_positions(t.ctypes.data, n, None, 0, 1, pos.ctypes.data, 3, out.ctypes.data) == E_ARG and np.all(out == 0xA5)
    assert L.acm_chars_positions(t.ctypes.data, n, None, 0, 1, pos.ctypes.data, 2, out.ctypes.data) == 0 and out.tolist()[:2] == [0, 8]
    out[:] = 0xA5
    assert L.acm_chars_positions(t.ctypes.data, n, None, 0, 7, pos.ctypes.data, 2, out.ctypes.data) == E_ARG and np.all(out == 0xA5)
    off = np.array([0, 5, 4, n], np.uint64)
    assert L.acm_chars_positions(t.ctypes.data, n, off.ctypes.data, 3, 1, pos.ctypes.data, 2, out.ctypes.data) == E_ARG and np.all(out == 0xA5)
    assert L.acm_chars_positions(None, n, None, 0, 1, pos.ctypes.data, 2, out.ctypes.data) == E_ARG and np.all(out == 0xA5)
    with pytest.raises(acm.ACMError):
        binding.chars_positions(text, [n + 1])
    with pytest.raises(KeyError):
        binding.chars_positions(text, [0], unit="graphemes")


def _loop_pair(kat, keywords):
    """(machine, oracle) over bytes under kat_cyclic_cmp8, which is no order (a < b < c < a; bytes are equal modulo 3):
    acm_flatten_classes refuses it, so no GPU plan can exist and the acm_scan_* calls run the caller loop on the host"""
    from oracle import pyoracle as po
    cmp = C.cast(kat.kat_cyclic_cmp8, C.c_void_p)
    m, o = acm.Machine(1, cmp=cmp), po.Oracle(1, po.MEYER85, cmp=cmp)
    for kw in keywords:
        m.add_keyword(kw)
        o.add_keyword(kw)
    m.set_symbol_bytes(1)
    return m, o


def test_machine_scan_chars_and_scan_str_on_the_host_loop(kat):
    m, o = _loop_pair(kat, cc.KEYWORDS)
    for seed, kind in ((5, "valid"), (6, "invalid")):
        text = cc.TEXT_KINDS[kind](seed, 2500)
        want_rec = o.scan(np.frombuffer(text, np.uint8))
        for unit in cc.UNITS:
            rec, start, length, edge = m.scan_chars(text, UNIT_NAMES[unit])
            assert m.scan_path == PATH_LOOP
            assert np.array_equal(rec, want_rec) and rec.size > 100
            want = cc.records_expected(text, want_rec, None, unit)
            assert np.array_equal(start, want[0]) and np.array_equal(length, want[1]) and np.array_equal(edge, want[2])
    # through the C call: one record too little room is an overflow that says what suffices; the path is recorded
    text = cc.valid_text(5, 2500)
    t = np.frombuffer(text, np.uint8)
    want_rec = o.scan(t)
    k = want_rec.size
    rec, start = np.zeros(k, cc.REC), np.zeros(k, np.uint64)
    n = C.c_uint64(0)

    def call(cap=k - 1, unit=1, start_ptr=start.ctypes.data):
        return m.L.acm_scan_chars(m.handle, t.ctypes.data, t.size, unit, rec.ctypes.data, start_ptr, None, None, cap, C.byref(n))
    assert call() == E_OVERFLOW and n.value == k and m.scan_path == PATH_LOOP
    assert call(cap=k) == 0 and np.array_equal(start, cc.records_expected(text, want_rec)[0])
    assert call(unit=0) == E_ARG and call(unit=3) == E_ARG and call(start_ptr=None) == E_ARG
    # a str caller: (start, stop, keyword_id, edge) in the indices of the str itself, in both units
    s = text.decode("utf-8")
    for unit in cc.UNITS:
        got = m.scan_str(s, UNIT_NAMES[unit])
        assert m.scan_path == PATH_LOOP and got.dtype == binding.STR_MATCH_DTYPE and got.size == k
        start, length, edge = cc.records_expected(text, want_rec, None, unit)
        assert np.array_equal(got["start"], start) and np.array_equal(got["stop"], start + length)
        assert np.array_equal(got["keyword_id"], want_rec["keyword_id"]) and np.array_equal(got["edge"], edge)
        # where a match covers whole characters its indices cut the str as its bytes cut the text
        for r, g in zip(want_rec[:400], got[:400]):
            if g["edge"] == 0:
                piece = text[int(r["end_pos"]) + 1 - int(r["length"]):int(r["end_pos"]) + 1].decode("utf-8")
                a, b = int(g["start"]), int(g["stop"])
                assert piece == (s[a:b] if unit == cc.CODEPOINTS else s.encode("utf-16-le")[2 * a:2 * b].decode("utf-16-le"))
    with pytest.raises(ValueError):
        acm.Machine(2).scan_str("abc")


def test_a_machine_over_wider_symbols_is_refused_on_the_host_loop():
    from tests.tally_cases import loop_machine
    h, keep = loop_machine([b"he", b"she"])                                  # 3-byte symbols
    L = acm.lib()
    text = np.zeros(30, np.uint8)
    rec, start, n = np.zeros(4, cc.REC), np.zeros(4, np.uint64), C.c_uint64(7)
    assert L.acm_scan_chars(h, text.ctypes.data, 10, 1, rec.ctypes.data, start.ctypes.data, None, None, 4, C.byref(n)) == E_ARG
    L.acm_release(h)


def test_plan_level_calls_refuse_a_missing_plan_before_they_touch_a_device():
    L = acm.lib()
    n = C.c_uint64(0)
    assert L.acm_gpu_chars_ruler_bytes(None, 100) == 0 and L.acm_gpu_chars_ruler_tmp_bytes(None, 100) == 0
    assert L.acm_gpu_chars_tmp_bytes(None, 10, 0) == 0 and L.acm_gpu_scan_chars_tmp_bytes(None, 10, 100, 0) == 0
    assert L.acm_gpu_chars_ruler_device(None, None, 0, None, 0, None, 0, None) == E_ARG
    assert L.acm_gpu_chars_records_device(None, None, 0, 0, None, 0, 1, None, None, 0, None, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_chars_positions_device(None, None, 0, None, 0, 1, None, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_chars_device(None, None, 0, 0, None, 0, 1, None, None, None, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_scan_chars_host(None, None, 0, 0, None, 0, 1, None, None, None, None, 0, C.byref(n)) == E_ARG


def _header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)            # comments mention functions too
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M)


def _declared():
    return set(re.findall(r"\b(acm_[a-z0-9_]+)\s*\(", _header_text()))


def test_export_list_is_the_header_and_apart_from_the_other_lists():
    L = acm.lib()
    assert _declared() == set(binding.CHARS_EXPORTS) and len(binding.CHARS_EXPORTS) == 12
    assert not set(binding.CHARS_EXPORTS) & (set(binding.EXPORTS) | set(binding.NEAR_EXPORTS) | set(binding.COOCCUR_EXPORTS))
    assert not any(w in name for name in binding.CHARS_EXPORTS for w in ("index", "cooccur", "near"))
    for name in binding.CHARS_EXPORTS:
        assert getattr(L, name) is not None, name
    nm = subprocess.run(["nm", "-D", "--defined-only", acm.library_path()], capture_output=True, check=True).stdout.decode()
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    assert set(s for s in exported if "chars" in s and s.startswith("acm_") and not s.startswith("acm_internal_")) == set(binding.CHARS_EXPORTS)
    tail = open(os.path.join(ROOT, "include", "acm_gpu.h")).read().split("#endif")[-1]
    assert tail.index('"acm_cooccur.h"') < tail.index('"acm_chars.h"') < tail.index('"acm_segment.h"')
    assert tail.strip().splitlines()[-1] == '#include "acm_segment.h"'
    whole = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "acm_gpu.h")).read(), flags=re.S)
    assert "chars" not in whole.replace('#include "acm_chars.h"', "").lower()
    assert (acm.ACM_CHARS_CODEPOINTS, acm.ACM_CHARS_UTF16, acm.ACM_CHARS_EDGE_START, acm.ACM_CHARS_EDGE_END, acm.ACM_CHARS_EDGE_BAD) == (1, 2, 1, 2, 4)
    src = open(HEADER).read()
    for name, value in (("CODEPOINTS", 1), ("UTF16", 2), ("EDGE_START", 1), ("EDGE_END", 2), ("EDGE_BAD", 4)):
        assert re.search(r"#define ACM_CHARS_%s %du\s" % (name, value), src), name


def test_signatures_agree_with_the_header():
    L = acm.lib()
    found = {}
    for ret, name, params in PROTOTYPE.findall(_header_text()):
        params = [] if params.strip() in ("", "void") else [c_class(p) for p in params.split(",")]
        assert name not in found
        found[name] = (c_class(ret, is_return=True), params)
    assert set(found) == set(binding.CHARS_EXPORTS)
    assert {name: (proto, signature(L, name)) for name, proto in found.items() if signature(L, name) != proto} == {}


def test_header_compiles_as_c11_and_every_declared_function_links(tmp_path):
    """include/acm_chars.h on its own after acm_gpu.h, and first of all"""
    for k, head in enumerate(('#include "aho_corasick.h"\n#include "acm_gpu.h"\n#include "acm_chars.h"\n', '#include "acm_chars.h"\n')):
        src = tmp_path / ("link_check_%d.c" % k)
        src.write_text(head + "int main(void){" + "".join("(void)%s;" % n for n in sorted(_declared())) +
                       "return (int)(ACM_CHARS_CODEPOINTS | ACM_CHARS_UTF16 | ACM_CHARS_EDGE_BAD) - 7;}\n")
        exe = str(tmp_path / ("link_check_%d" % k))
        p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                            "-L", os.path.dirname(acm.library_path()), "-lac75_amd", "-Wl,-rpath," + os.path.dirname(acm.library_path())],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
