"""Keyword chains with bounded gaps on the host (acm_chains_check, acm_chains_records, the host path of
acm_scan_chains, ChainSet.from_specs).  The expected answer is always the definition of CHAINS in plain Python
over the ORACLE's records (tests/chain_cases.py: every start of every embedding, kept as a set) and, for byte
text, a second derivation from the text alone with `re` -- never the library's own scan or join.  All
comparisons are exact, order included.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.chain_cases import (CASE_CHAINS, CASE_CUT, CASE_KEYWORDS, CASE_TEXT, brute, case_facts, chain_terms, chains, chains_by_re, fixed_offset_patterns,
                               oracle_records, random_case)
from tests.pattern_cases import patterns
from tests.words_cases import loop_machine8, sym8

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
PATH_LOOP = 3
GAP_MAX = 1 << 20


def _same(got, want, what=None):
    assert got.size == want.size and np.array_equal(np.asarray(got).astype(po.RECORD_DTYPE), want), (what, got.size, want.size, got[:8], want[:8])


def _check(chain_list, n_keywords, terms=None, chain_ptr=None, n_chains=None):
    """acm_chains_check on lists of terms, or on raw arrays"""
    cs = binding.ChainSet(chain_list)
    t = cs.terms if terms is None else np.asarray(terms, np.uint32).reshape(-1, 3)
    p = cs.chain_ptr if chain_ptr is None else np.asarray(chain_ptr, np.uint64)
    n = cs.n_chains if n_chains is None else n_chains
    return acm.lib().acm_chains_check(t.ctypes.data if t.size else None, p.ctypes.data, n, n_keywords)


def test_chains_check_names_every_argument_error():
    ok = [[(0, 0, 0), (1, 2, 40)], [(1, 0, 0)]]
    assert _check(ok, 2) == 0
    assert _check([], 0) == 0                                                    # no chain is a set
    assert _check(ok, 2, chain_ptr=[0, 2, 2], n_chains=2) == E_ARG               # a chain without terms
    assert _check([[(0, 0, 0)] + [(0, 0, 1)] * 15], 1) == 0                      # 16 terms: the most
    assert _check([[(0, 0, 0)] + [(0, 0, 1)] * 16], 1) == E_ARG                  # 17 terms
    assert _check([[(0, 0, 0), (0, 3, 2)]], 1) == E_ARG                          # gap_min > gap_max
    assert _check([[(0, 0, 0), (0, GAP_MAX, GAP_MAX)]], 1) == 0                  # gap_max = 2^20: the widest
    assert _check([[(0, 0, 0), (0, 0, GAP_MAX + 1)]], 1) == E_ARG                # gap_max > 2^20
    assert _check([[(0, 0, 1)]], 1) == E_ARG and _check([[(0, 1, 1)]], 1) == E_ARG   # a first term whose gaps are not 0, 0
    assert _check([[(0, 0, 0)], [(0, 0, 2), (0, 0, 0)]], 1) == E_ARG             # (of a later chain as well)
    assert _check(ok, 1) == E_ARG                                                # keyword_id >= n_keywords
    assert _check(ok, 2, chain_ptr=[0, 3, 2], n_chains=2) == E_ARG               # chain_ptr decreases
    assert _check(ok, 2, chain_ptr=[1, 2, 3], n_chains=2) == E_ARG               # chain_ptr does not begin with 0
    assert _check(ok, 2, n_chains=1 << 31) == E_ARG                              # (checked before chain_ptr is read that far)
    assert _check([[(0, 0, 0)]], 1, chain_ptr=[0, 1 << 31], n_chains=1) == E_ARG  # 2^31 terms (checked before terms[] is read)
    assert acm.lib().acm_chains_check(None, None, 0, 0) == E_ARG
    with pytest.raises(acm.ACMError):
        binding.ChainSet(ok).check(1)
    binding.ChainSet(ok).check(2)


def test_the_two_derivations_agree_on_the_fixed_case_and_the_case_is_not_trivial():
    rec = oracle_records(CASE_KEYWORDS, CASE_TEXT)
    for offsets in (None, [0, CASE_CUT, len(CASE_TEXT)]):
        _same(chains(rec, CASE_CHAINS, len(CASE_TEXT), offsets), chains_by_re(CASE_KEYWORDS, CASE_CHAINS, CASE_TEXT, offsets), offsets)
    per, ties, several, ruled_out, lost = case_facts(CASE_KEYWORDS, CASE_CHAINS, CASE_TEXT, CASE_CUT)
    print("records %d, matches per chain %s, ties %d, ends with several starts %d, ruled out by a middle gap %d, lost to the cut %d"
          % (rec.size, per, ties, several, ruled_out, lost))
    assert min(per) >= 2 and ties >= 2 and several >= 1 and ruled_out >= 1 and lost >= 1


def test_chains_records_on_the_fixed_case():
    text = CASE_TEXT
    rec = oracle_records(CASE_KEYWORDS, text)
    nk = len(CASE_KEYWORDS)
    want = chains(rec, CASE_CHAINS, len(text))
    _same(binding.chains_records(rec, CASE_CHAINS, len(text), n_keywords=nk), want)
    off = np.array([0, CASE_CUT, len(text)], np.uint64)
    _same(binding.chains_records(rec, CASE_CHAINS, len(text), offsets=off, n_keywords=nk), chains(rec, CASE_CHAINS, len(text), off))
    # count-only, overflow (nothing written), the exact room
    L = acm.lib()
    cs = binding.ChainSet(CASE_CHAINS)
    n = C.c_uint64(0)

    def call(out, cap, records=rec, n_symbols=len(text), pos_base=0, off=None, n_texts=0):
        return L.acm_chains_records(records.ctypes.data, records.size, n_symbols, pos_base, off.ctypes.data if off is not None else None, n_texts,
                                    *cs.args(), nk, out.ctypes.data if out is not None else None, cap, C.byref(n))
    assert call(None, 0) == 0 and n.value == want.size
    out = np.zeros(want.size, po.RECORD_DTYPE)
    out["end_pos"] = 0x5555
    n.value = 0
    assert call(out, want.size - 1) == E_OVERFLOW and n.value == want.size and np.all(out["end_pos"] == 0x5555)
    assert call(out, want.size) == 0 and n.value == want.size
    _same(out, want)
    # nonzero pos_base
    shifted, moved = rec.copy(), want.copy()
    shifted["end_pos"] += 1 << 40
    moved["end_pos"] += 1 << 40
    _same(chains(shifted, CASE_CHAINS, len(text), pos_base=1 << 40), moved)
    _same(binding.chains_records(shifted, CASE_CHAINS, len(text), pos_base=1 << 40, n_keywords=nk), moved)
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


def test_chains_records_equals_the_definition_and_re_on_300_random_cases():
    rng = np.random.default_rng(1975)
    matches = ties = cut_trials = 0
    for trial in range(300):
        kws, chain_list, text, offsets = random_case(rng)
        rec = oracle_records(kws, text)
        want = chains(rec, chain_list, len(text), offsets)
        _same(want, chains_by_re(kws, chain_list, text, offsets), (trial, "the two derivations"))
        got = binding.chains_records(rec, chain_list, len(text), offsets=offsets, n_keywords=len(kws))
        _same(got, want, (trial, kws, chain_list, text, offsets))
        if offsets.size == 2:                                                    # one text: offsets NULL says the same
            _same(binding.chains_records(rec, chain_list, len(text), n_keywords=len(kws)), want, trial)
        matches += want.size
        ties += int(np.count_nonzero(want["end_pos"][1:] == want["end_pos"][:-1]))
        cut_trials += offsets.size > 2
    print("matches %d, ties in end_pos %d, trials with cuts %d" % (matches, ties, cut_trials))
    assert matches > 1000 and ties > 100 and cut_trials > 100


def test_gap_boundaries_and_special_shapes():
    kws = [b"ab", b"bc", b"x", b"y"]
    chain = [[(2, 0, 0), (3, 2, 4)]]                                              # x .{2,4} y

    def run(text, chain_list=chain):
        rec = oracle_records(kws, text)
        want = chains(rec, chain_list, len(text))
        _same(want, chains_by_re(kws, chain_list, text), text)
        _same(binding.chains_records(rec, chain_list, len(text), n_keywords=len(kws)), want, text)
        return [tuple(int(v) for v in r) for r in want]
    assert run(b"x.y") == [] and run(b"x..y") == [(3, 4, 0)] and run(b"x....y") == [(5, 6, 0)] and run(b"x.....y") == []
    assert run(b"xy", [[(2, 0, 0), (3, 0, 0)]]) == [(1, 2, 0)] and run(b"x.y", [[(2, 0, 0), (3, 0, 0)]]) == []
    assert run(b"abc", [[(0, 0, 0), (1, 0, 0)]]) == []                            # ab and bc overlap: no chain at gap 0
    assert run(b"abbc", [[(0, 0, 0), (1, 0, 0)]]) == [(3, 4, 0)]
    assert run(b"x.y", [[(2, 0, 0), (3, 0, 9)]]) == [(2, 3, 0)]                   # the window's lower end clamps at the buffer's first symbol
    assert run(b"y.x", [[(2, 0, 0), (3, 0, 9)]]) == []                            # a second term at index 0 has nothing in front
    assert run(b"xx.y", [[(2, 0, 0), (3, 0, 9)]]) == [(3, 3, 0)]                  # the latest start
    assert run(b"x.x", [[(2, 0, 0)]]) == [(0, 1, 0), (2, 1, 0)]                   # a chain of one term: its keyword's records
    # a chain whose gaps are all fixed is the pattern with those offsets
    text = b"ab.bc abxbc abbc ab..bc xabybc"
    fixed = [[(0, 0, 0), (1, 1, 1)], [(2, 0, 0), (0, 0, 0), (3, 0, 0)], [(0, 0, 0), (1, 0, 0)]]
    rec = oracle_records(kws, text)
    want = chains(rec, fixed, len(text))
    _same(want, patterns(rec, fixed_offset_patterns(kws, fixed), len(text)))
    _same(binding.chains_records(rec, fixed, len(text), n_keywords=len(kws)), want)
    assert want.size >= 4
    # symbols wider than a byte
    words = [[70000, 70001], [5]]
    t4 = np.array([70000, 70001, 9, 9, 5, 70000, 70001, 5, 5], np.uint32)
    wide = [[(0, 0, 0), (1, 0, 2)]]
    rec4 = brute(words, t4)
    want = chains(rec4, wide, t4.size)
    assert [tuple(int(v) for v in r) for r in want] == [(4, 5, 0), (7, 3, 0), (8, 4, 0)]
    _same(binding.chains_records(rec4, wide, t4.size, n_keywords=2), want)


def _scan_chains(h, text8, chain_list, cap, offsets=None):
    L = acm.lib()
    cs = binding.ChainSet(chain_list)
    out = np.zeros(max(cap, 1), po.RECORD_DTYPE)
    n = C.c_uint64(0)
    off = np.ascontiguousarray(offsets, np.uint64) if offsets is not None else None
    rc = L.acm_scan_chains(h, text8.ctypes.data if text8.size else None, text8.size, off.ctypes.data if off is not None else None,
                           off.size - 1 if off is not None else 0, *cs.args(), out.ctypes.data if cap else None, cap, C.byref(n))
    return rc, int(n.value), out


def test_acm_scan_chains_on_the_host_loop():
    L = acm.lib()
    text = CASE_TEXT
    want = chains_by_re(CASE_KEYWORDS, CASE_CHAINS, text)
    h, keep = loop_machine8(CASE_KEYWORDS)
    assert L.acm_scan_path(h) == 0
    rc, n, out = _scan_chains(h, sym8(text), CASE_CHAINS, want.size)
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    _same(out[:n], want)
    # too little room: the count that suffices comes back, the repeat succeeds; no room at all only counts
    rc, n, out = _scan_chains(h, sym8(text), CASE_CHAINS, want.size - 1)
    assert rc == E_OVERFLOW and n == want.size
    rc, n, out = _scan_chains(h, sym8(text), CASE_CHAINS, 0)
    assert rc == 0 and n == want.size
    # a batch: the same buffer cut into texts, empty ones among them
    offsets = np.array([0, 0, CASE_CUT, 70, 70, len(text)], np.uint64)
    cut = chains_by_re(CASE_KEYWORDS, CASE_CHAINS, text, offsets)
    assert 0 < cut.size < want.size
    rc, n, out = _scan_chains(h, sym8(text), CASE_CHAINS, want.size, offsets=offsets)
    assert rc == 0
    _same(out[:n], cut)
    rc, n, out = _scan_chains(h, sym8(b""), CASE_CHAINS, 4)
    assert (rc, n) == (0, 0)
    # argument errors on this path too
    assert _scan_chains(h, sym8(text), [[(len(CASE_KEYWORDS), 0, 0)]], want.size)[0] == E_ARG
    assert _scan_chains(h, sym8(text), [[(0, 0, 0), (1, 5, 4)]], want.size)[0] == E_ARG
    assert _scan_chains(h, sym8(text), CASE_CHAINS, want.size, offsets=[0, 7, 5, len(text)])[0] == E_ARG
    L.acm_release(h)


def test_from_specs_inserts_missing_keywords_and_reuses_ids():
    m = acm.Machine(1)
    m.add_keyword(b"HTTP")
    m.add_keyword(b"GET")
    cs = binding.ChainSet.from_specs(m, [[b"GET", (2, 30), b"HTTP"], [b"Host", (0, 1), b":", (0, 4), b":"], [b"GET"]])
    assert [bytes(m.keyword(k)[0]) for k in range(m.nb_keywords)] == [b"HTTP", b"GET", b"Host", b":"] and cs.n_keywords == 4
    assert chain_terms(cs) == [[(1, 0, 0), (0, 2, 30)], [(2, 0, 0), (3, 0, 1), (3, 0, 4)], [(1, 0, 0)]]
    assert cs.chain_ptr.tolist() == [0, 2, 5, 6] and cs.n_chains == 3
    for bad in ([[b"a", (0, 1)]], [[]], [[b"a", (0, 1, 2), b"b"]], [[b"", (0, 1), b"b"]]):
        with pytest.raises(ValueError):
            binding.ChainSet.from_specs(m, bad)
    words = [bytes(m.keyword(k)[0]) for k in range(m.nb_keywords)]
    got = binding.chains_records(oracle_records(words, CASE_TEXT), cs, len(CASE_TEXT))
    _same(got, chains_by_re(words, chain_terms(cs), CASE_TEXT))
    assert got.size > 8
    m4 = acm.Machine(4)                                                          # symbols wider than a byte
    cs4 = binding.ChainSet.from_specs(m4, [[np.array([70000, 70001], np.uint32), (0, 2), np.array([5], np.uint32)]])
    assert m4.nb_keywords == 2 and chain_terms(cs4) == [[(0, 0, 0), (1, 0, 2)]]
