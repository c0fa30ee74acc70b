"""Keyword patterns with don't-care gaps on the host (acm_patterns_check, acm_patterns_records, the host path of
acm_scan_patterns, PatternSet.from_templates).  The expected answer is always the definition of PATTERNS in
plain Python over the ORACLE's or tests/brute.py's records (tests/pattern_cases.py) and, for byte text, a
second derivation from the text alone with `re` lookaheads -- never the library's own scan or join.  All
comparisons are exact, order included.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.pattern_cases import (as_records, brute, compile_templates, oracle_records, patterns, patterns_by_re, random_case)
from tests.words_cases import loop_machine8, sym8

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
PATH_LOOP = 3


def _same(got, want, what=None):
    assert got.size == want.size and np.array_equal(np.asarray(got).astype(po.RECORD_DTYPE), want), (what, got.size, want.size, got[:8], want[:8])


def _check(pats, n_keywords, terms=None, pat_ptr=None, n_patterns=None):
    """acm_patterns_check on lists of terms, or on raw arrays"""
    ps = binding.PatternSet(pats)
    t = ps.terms if terms is None else np.asarray(terms, np.uint32).reshape(-1, 3)
    p = ps.pat_ptr if pat_ptr is None else np.asarray(pat_ptr, np.uint64)
    n = ps.n_patterns if n_patterns is None else n_patterns
    return acm.lib().acm_patterns_check(t.ctypes.data if t.size else None, p.ctypes.data, n, n_keywords)


def test_patterns_check_names_every_argument_error():
    ok = [[(0, 0, 2), (1, 3, 1)], [(1, 1, 1)]]
    assert _check(ok, 2) == 0
    assert _check([], 0) == 0                                                    # no pattern is a set
    assert _check(ok, 2, pat_ptr=[0, 2, 2], n_patterns=2) == E_ARG               # a pattern without terms
    assert _check([[(0, 0, 0)]], 1) == E_ARG                                     # length 0
    assert _check([[(0, (1 << 31) - 2, 1)]], 1) == 0                             # offset + length = 2^31 - 1: the last that fits
    assert _check([[(0, (1 << 31) - 1, 1)]], 1) == E_ARG                         # offset + length = 2^31
    assert _check([[(0, 0xFFFFFFFF, 0xFFFFFFFF)]], 1) == E_ARG                   # (no 32-bit wrap-around)
    assert _check(ok, 1) == E_ARG                                                # keyword_id >= n_keywords
    assert _check(ok, 2, pat_ptr=[0, 3, 2], n_patterns=2) == E_ARG               # pat_ptr decreases
    assert _check(ok, 2, pat_ptr=[1, 2, 3], n_patterns=2) == E_ARG               # pat_ptr does not begin with 0
    assert _check(ok, 2, n_patterns=1 << 31) == E_ARG                            # (checked before pat_ptr is read that far)
    assert _check([[(0, 0, 1)]], 1, pat_ptr=[0, 1 << 31], n_patterns=1) == E_ARG  # 2^31 terms (checked before terms[] is read)
    assert acm.lib().acm_patterns_check(None, None, 0, 0) == E_ARG
    with pytest.raises(acm.ACMError):
        binding.PatternSet(ok).check(1)
    binding.PatternSet(ok).check(2)


def test_patterns_records_equals_the_definition_and_re_on_400_random_template_sets():
    rng = np.random.default_rng(1975)
    matches = ties = cut_texts = 0
    for trial in range(400):
        templates, text, offsets = random_case(rng)
        kws, pats = compile_templates(templates)
        rec = oracle_records([bytes(k) for k in kws], text)
        want = patterns(rec, pats, len(text), offsets)
        _same(want, patterns_by_re(templates, text, offsets), (trial, "the two derivations"))
        got = binding.patterns_records(rec, pats, len(text), offsets=offsets, n_keywords=len(kws))
        _same(got, want, (trial, templates, text, offsets))
        if offsets.size == 2:                                                    # one text: offsets NULL says the same
            _same(binding.patterns_records(rec, pats, len(text), n_keywords=len(kws)), want, trial)
        matches += want.size
        ties += int(np.count_nonzero(want["end_pos"][1:] == want["end_pos"][:-1]))
        cut_texts += offsets.size > 2
    print("matches %d, ties in end_pos %d, trials with cuts %d" % (matches, ties, cut_texts))
    assert matches > 2000 and ties > 100 and cut_texts > 100


# (the novel's file separates words by tabs: the first two templates, with a blank, are rare in it, so the same with a tab are added)
NOVEL_TEMPLATES = [b"M??. Dalloway", b"th? ", b"?he", b"Clarissa", b"M??.\tDalloway", b"th?\t"]


def test_patterns_records_on_the_novel(novel_bytes):
    text = novel_bytes[:6000]
    kws, pats = compile_templates(NOVEL_TEMPLATES)
    rec = oracle_records([bytes(k) for k in kws], text)
    want = patterns(rec, pats, len(text))
    _same(want, patterns_by_re(NOVEL_TEMPLATES, text), "the two derivations")
    per = np.bincount(want["keyword_id"], minlength=len(NOVEL_TEMPLATES))
    print("records %d, matches per template %s" % (rec.size, per.tolist()))
    assert np.all(per[2:] > 0) and len(set(per[2:].tolist())) == 4
    _same(binding.patterns_records(rec, pats, len(text), n_keywords=len(kws)), want)
    # count-only, overflow (nothing written), the exact room
    L = acm.lib()
    ps = binding.PatternSet(pats)
    n = C.c_uint64(0)

    def call(out, cap, records=rec, n_symbols=len(text), pos_base=0, off=None, n_texts=0):
        return L.acm_patterns_records(records.ctypes.data, records.size, n_symbols, pos_base, off.ctypes.data if off is not None else None, n_texts,
                                      *ps.args(), len(kws), out.ctypes.data if out is not None else None, cap, C.byref(n))
    assert call(None, 0) == 0 and n.value == want.size
    out = np.zeros(want.size, po.RECORD_DTYPE)
    out["end_pos"] = 0x5555
    n.value = 0
    assert call(out, want.size - 1) == E_OVERFLOW and n.value == want.size and np.all(out["end_pos"] == 0x5555)
    assert call(out, want.size) == 0 and n.value == want.size
    _same(out, want)
    # nonzero pos_base
    shifted = rec.copy()
    shifted["end_pos"] += 1 << 40
    moved = want.copy()
    moved["end_pos"] += 1 << 40
    _same(patterns(shifted, pats, len(text), pos_base=1 << 40), moved)
    _same(binding.patterns_records(shifted, pats, len(text), pos_base=1 << 40, n_keywords=len(kws)), moved)
    # records outside [pos_base, pos_base + n_symbols), their end or their start, or of length 0; offsets that break the contract
    assert call(out, want.size, records=shifted) == E_ARG                        # ends behind the buffer
    assert call(out, want.size, n_symbols=int(rec["end_pos"][-1])) == E_ARG      # the last record ends at n_symbols
    assert call(out, want.size, pos_base=1) == E_ARG                             # the first record begins in front of pos_base
    zero = rec.copy()
    zero["length"][3] = 0
    assert call(out, want.size, records=zero) == E_ARG
    for off in ([0, 10, 5, len(text)], [1, len(text)], [0, len(text) - 1]):
        assert call(out, want.size, off=np.array(off, np.uint64), n_texts=len(off) - 1) == E_ARG
    _same(out, want)                                                             # nothing was written by the refused calls


def test_a_term_with_a_wrong_length_never_holds_and_terms_may_overlap():
    text = b"xabcabcx abcab"
    kws = [b"abc", b"ab", b"bc", b"c"]
    rec = oracle_records(kws, text)
    # `abc` said to be 2 symbols long: no record (end, 2, 0) exists, also not where `ab` (end, 2, 1) does
    assert patterns(rec, [[(0, 0, 2)]], len(text)).size == 0
    assert binding.patterns_records(rec, [[(0, 0, 2)]], len(text), n_keywords=4).size == 0
    # overlapping terms in any order, a leading don't-care, an anchor tie (the first of two terms that end together)
    pats = [[(2, 1, 2), (1, 0, 2)], [(3, 3, 1), (1, 1, 2)], [(3, 2, 1), (0, 0, 3), (2, 1, 2)]]
    want = patterns(rec, pats, len(text))
    _same(want, patterns_by_re([b"abc", b"?abc", b"abc"], text))
    assert want.size == 3 + 3 + 3
    _same(binding.patterns_records(rec, pats, len(text), n_keywords=4), want)


def _scan_patterns(h, text8, pats, cap, offsets=None):
    L = acm.lib()
    ps = binding.PatternSet(pats)
    out = np.zeros(max(cap, 1), po.RECORD_DTYPE)
    n = C.c_uint64(0)
    off = np.ascontiguousarray(offsets, np.uint64) if offsets is not None else None
    rc = L.acm_scan_patterns(h, text8.ctypes.data if text8.size else None, text8.size, off.ctypes.data if off is not None else None,
                             off.size - 1 if off is not None else 0, *ps.args(), out.ctypes.data if cap else None, cap, C.byref(n))
    return rc, int(n.value), out


def test_acm_scan_patterns_on_the_host_loop(novel_bytes):
    L = acm.lib()
    text = novel_bytes[:6000]
    kws, pats = compile_templates(NOVEL_TEMPLATES)
    want = patterns_by_re(NOVEL_TEMPLATES, text)
    h, keep = loop_machine8([bytes(k) for k in kws])
    assert L.acm_scan_path(h) == 0
    rc, n, out = _scan_patterns(h, sym8(text), pats, want.size)
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    _same(out[:n], want)
    # too little room: the count that suffices comes back, the repeat succeeds; no room at all only counts
    rc, n, out = _scan_patterns(h, sym8(text), pats, want.size - 1)
    assert rc == E_OVERFLOW and n == want.size
    rc, n, out = _scan_patterns(h, sym8(text), pats, 0)
    assert rc == 0 and n == want.size
    # a batch: the same buffer cut into texts, one cut inside a `Mrs. Dalloway`
    at = text.index(b"Mrs.\tDalloway")
    offsets = np.array([0, 0, at + 5, 3000, 3000, len(text)], np.uint64)
    cut = patterns_by_re(NOVEL_TEMPLATES, text, offsets)
    assert 0 < cut.size < want.size
    rc, n, out = _scan_patterns(h, sym8(text), pats, want.size, offsets=offsets)
    assert rc == 0
    _same(out[:n], cut)
    rc, n, out = _scan_patterns(h, sym8(b""), pats, 4)
    assert (rc, n) == (0, 0)
    # this call knows the machine: a term whose length is not its keyword's is an argument error
    wrong = [list(p) for p in pats]
    k, o, l = wrong[0][0]
    wrong[0][0] = (k, o, l + 1)
    assert _scan_patterns(h, sym8(text), wrong, want.size)[0] == E_ARG
    assert _scan_patterns(h, sym8(text), [[(len(kws), 0, 1)]], want.size)[0] == E_ARG
    assert _scan_patterns(h, sym8(text), pats, want.size, offsets=[0, 7, 5, len(text)])[0] == E_ARG
    L.acm_release(h)


def test_from_templates_cuts_runs_reuses_ids_and_refuses_trailing_dont_cares():
    m = acm.Machine(1)
    m.add_keyword(b"C8A1")
    m.add_keyword(b"E2")
    templates = [b"E234?C8A1", b"?E2", b"E2?E234", b"E2"]
    ps = binding.PatternSet.from_templates(m, templates, wildcard=b"?")
    kws, pats = compile_templates(templates, keywords=[tuple(b"C8A1"), tuple(b"E2")])
    assert m.nb_keywords == 3 == len(kws) and ps.n_keywords == 3                 # only `E234` is new
    assert [bytes(m.keyword(k)[0]) for k in range(3)] == [b"C8A1", b"E2", b"E234"]
    assert ps.terms.tolist() == [list(t) for p in pats for t in p] == [[2, 0, 4], [0, 5, 4], [1, 1, 2], [1, 0, 2], [2, 3, 4], [1, 0, 2]]
    assert ps.pat_ptr.tolist() == [0, 2, 3, 5, 6] and ps.n_patterns == 4
    ps2 = binding.PatternSet.from_templates(m, [b"34??34"], wildcard=ord("?"))   # one new run, used twice
    assert m.nb_keywords == 4 and ps2.terms.tolist() == [[3, 0, 2], [3, 4, 2]]
    assert binding.PatternSet.from_templates(m, [b"a?b"]).terms.tolist() == [[4, 0, 3]]   # no wildcard given: `?` is a symbol
    for bad in ([b"ab?"], [b""], [b"??"]):
        with pytest.raises(ValueError):
            binding.PatternSet.from_templates(m, bad, wildcard=b"?")
    # what the set matches is what the templates say
    m = acm.Machine(1)
    templates = [b"a?c", b"ab?d", b"?bc"]
    ps = binding.PatternSet.from_templates(m, templates, wildcard=b"?")
    text = b"abcd abd abxd xbc"
    words = [bytes(m.keyword(k)[0]) for k in range(m.nb_keywords)]
    got = binding.patterns_records(oracle_records(words, text), ps, len(text))
    _same(got, patterns_by_re(templates, text))
    # symbols wider than a byte
    m4 = acm.Machine(4)
    ps4 = binding.PatternSet.from_templates(m4, [np.array([70000, 0, 70001], np.uint32)], wildcard=0)
    t4 = np.array([70000, 5, 70001, 70000, 70001], np.uint32)
    words = [list(m4.keyword(k)[0]) for k in range(m4.nb_keywords)]
    got = binding.patterns_records(brute(words, t4), ps4, t4.size)
    assert [tuple(int(x) for x in r) for r in got] == [(2, 3, 0)]
