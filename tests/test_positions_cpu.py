"""Record positions across the 2^32 carry and with bit 63 set, without a GPU: the host C functions of every
family (through `binding` where a wrapper exists), the flattened-table walker of the tests, and the checks
that the cases of test_positions_gpu.py cannot pass trivially.  The expected answer is always the family's
Python definition over the ORACLE's records at pos_base = 0, then translated (tests/position_cases.py)."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests import position_cases as pc
from tests.flatwalk import walk_csr
from tests.position_cases import (BATCH_FAMILIES, CONTEXT_AFTER, CONTEXT_BEFORE, FAMILIES, NAMES, TEXT_FAMILIES, bases, boundary_of, breach_positions, inputs, moved,
                                  same, sets_of, thirds, want_of)
from tests.tally_cases import KINDS

E_ARG = binding.ACM_GPU_E_ARG


def host(family, sb, records, base, offsets=None):
    """the family's host C function on `records` (positions base + index): (records or None, rest, tok_start or None)"""
    text = inputs(family, sb)[0]
    tset, nk = sets_of(family, sb)
    if family == "select":
        return binding.select_records(records), (), None
    if family == "segment":
        out, sums = binding.segment_records(records, pc.SEGMENT_COST, pc.SEGMENT_GAP)
        return out, (np.array(sums, np.uint64),), None
    if family == "words":
        return binding.words_records(text, records, offsets, pc.ranges_of(sb), pos_base=base), (), None
    if family == "context":
        s = binding.context_records(text, records, offsets, CONTEXT_BEFORE, CONTEXT_AFTER, pos_base=base)
        return None, (s.snip_lo, s.out_offsets, s.snip_text, s.rec_snip, s.rec_at, s.out), None
    if family == "replace":
        assert offsets is None
        return None, (binding.replace_records(text, records, pc.replacements_of(sb), pos_base=base), None), None
    if family == "tokens":
        t = binding.tokens_records(text, records, offsets, mode="run", gap_base=pc.TOKEN_GAP_BASE, pos_base=base)
        return None, (t.ids, t.length) + ((t.first,) if offsets is not None else ()), t.start
    if family == "patterns":
        return binding.patterns_records(records, tset, text.size, offsets, base, nk), (), None
    if family == "chains":
        return binding.chains_records(records, tset, text.size, offsets, base, nk), (), None
    fn = {"approx": binding.approx_records, "edit": binding.edit_records, "templates": binding.templates_records}[family]
    out, dist = fn(records, tset, text, offsets, base, nk)
    return out, (dist,), None


def _cases():
    return [(f, sb) for f in FAMILIES for sb in ((1, 4) if f in TEXT_FAMILIES else (1,))]


@pytest.mark.parametrize("family,sb", _cases())
def test_case_straddles_the_boundary_and_is_not_trivial(family, sb):
    """the three conditions on the records and on the expected output, from the oracle alone; the output is
    neither empty nor everything"""
    c = boundary_of(family, sb)
    w = want_of(family, sb)
    n_out = w.extent[0].size
    print(family, sb, "c = %d, records %d, outputs %d" % (c, inputs(family, sb)[1].size, n_out))
    assert n_out >= 6
    if family in ("select", "segment", "words", "context"):                     # a proper part of the records, snippets that merge some
        assert n_out < w.rec.size
    if family in BATCH_FAMILIES:
        n = inputs(family, sb)[0].size
        for off in (thirds(n), thirds(n, c)):
            cut = want_of(family, sb, off)
            assert cut.extent[0].size >= 4
            below, above = np.count_nonzero(cut.extent[1] < c), np.count_nonzero(cut.extent[1] >= c)
            assert below and above, (family, off)
        # a boundary between two texts cannot lie inside an output; with the carry INSIDE a text one does
        inside = want_of(family, sb, thirds(n))
        assert np.any((inside.extent[0] < c) & (c <= inside.extent[1])), family


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family,sb", _cases())
def test_host_functions_at_the_carry(family, sb, name):
    c = boundary_of(family, sb)
    base = bases(c)[name]
    w = want_of(family, sb)
    same(host(family, sb, moved(w.rec, base), base), w.at(base), (family, sb, name))
    if family in BATCH_FAMILIES:
        n = inputs(family, sb)[0].size
        for off in (thirds(n), thirds(n, c)):                                    # the carry inside a text, and on a text boundary
            cut = want_of(family, sb, off)
            same(host(family, sb, moved(cut.rec, base), base, off), cut.at(base), (family, sb, name, off.tolist()))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family", [f for f in FAMILIES if f not in ("select", "segment")])
def test_host_functions_refuse_a_wrong_high_word(family, name):
    """a valid set with ONE stranger mixed in: a position whose low word is valid and whose high word is not
    (in_range - 2^32, in_range + 2^32), pos_base - 1, pos_base + n_symbols.  Every host function refuses such
    a set with ACM_GPU_E_ARG, as its own test at pos_base 1000 expects.  (acm_select_records and
    acm_segment_records take no range: there is nothing to breach.)"""
    sb = 1
    c = boundary_of(family, sb)
    base = bases(c)[name]
    w = want_of(family, sb)
    text = inputs(family, sb)[0]
    good = moved(w.rec, base)
    same(host(family, sb, good, base), w.at(base), (family, name))
    model = good[good.size // 2]
    for pos in breach_positions(base, text.size, int(w.rec["end_pos"][w.rec.size // 2])):
        stranger = np.array([(pos, model["length"], model["keyword_id"])], po.RECORD_DTYPE)
        mixed = pc.canonical(np.concatenate([good, stranger]))
        with pytest.raises(acm.ACMError) as e:
            host(family, sb, mixed, base)
        assert e.value.code == E_ARG, (family, name, hex(pos))


@pytest.mark.parametrize("name", KINDS)
def test_core_scan_cases_straddle_and_the_table_walker_agrees(monkeypatch, kat, novel_bytes, name):
    """the 64 Ki symbol texts of test_positions_gpu.py: the conditions on their records, and tests/flatwalk's
    walk of the flattened tables at both bases, whole and from a cut three symbols in front of the boundary"""
    m, o, text, c, rec = pc.scan_case(name, monkeypatch, kat, novel_bytes)
    if name in ("classes", "u64"):
        return                                                                   # (tables over classes and over interned symbols: no walker for them)
    flat = m.flatten()
    for bname in NAMES:
        base = bases(c)[bname]
        for emit_from in (0, c - 3):
            want = moved(rec[rec["end_pos"] >= emit_from], base)
            got = walk_csr(flat, text, emit_from=emit_from, pos_base=base)
            assert got.size == want.size and np.array_equal(got, want), (name, bname, emit_from)
