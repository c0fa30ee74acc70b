"""Keywords with up to k mismatches on the host (acm_approx_check, acm_approx_split, acm_approx_records, the host
path of acm_scan_approx, ApproxSet.from_targets).  The expected answer is always the definition of APPROX in plain
Python over the ORACLE's or tests/brute.py's records (tests/approx_cases.py) and, for canonical cuts, a second
derivation from the text alone (a brute-force Hamming scan) -- never the library's own scan or join.  All
comparisons are exact, order and distances included.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.approx_cases import approx, brute, compile_targets, hamming_scan, oracle_records, random_case, same, split

E_ARG, E_OVERFLOW, E_INELIGIBLE = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, binding.ACM_GPU_E_INELIGIBLE
PATH_LOOP = 3


def _check(targets, k, terms, n_keywords, spell_off=None, tgt_ptr=None, n_targets=None):
    """acm_approx_check on lists, or on raw arrays"""
    a = binding.ApproxSet(targets, k, terms)
    so = a.spell_off if spell_off is None else np.asarray(spell_off, np.uint64)
    tp = a.tgt_ptr if tgt_ptr is None else np.asarray(tgt_ptr, np.uint64)
    n = a.n_targets if n_targets is None else n_targets
    return acm.lib().acm_approx_check(so.ctypes.data, a.k.ctypes.data if a.k.size else None, a.terms.ctypes.data if a.terms.size else None,
                                      tp.ctypes.data, n, n_keywords)


def test_approx_check_names_every_argument_error():
    tg, ok = [b"abcd", b"xyz"], [[(0, 0, 2), (1, 2, 2)], [(1, 1, 2)]]
    assert _check(tg, 1, ok, 2) == 0
    assert _check([], 0, [], 0) == 0                                             # no target is a set
    assert _check(tg, 1, ok, 2, tgt_ptr=[0, 2, 2]) == E_ARG                      # a target without terms
    assert _check(tg, 1, ok, 2, spell_off=[0, 4, 4]) == E_ARG                    # L_w == 0
    assert _check(tg, 1, ok, 2, spell_off=[0, 1 << 31, (1 << 31) + 3]) == E_ARG  # L_w == 2^31
    assert _check(tg, [1, 255], ok, 2) == 0
    assert _check(tg, [1, 256], ok, 2) == E_ARG                                  # k > 255
    assert _check(tg, 1, [[(0, 0, 0)], [(1, 1, 2)]], 2) == E_ARG                 # length 0
    assert _check(tg, 1, [[(0, 0, 4)], [(1, 1, 2)]], 2) == 0                     # offset + length == L_w: the last that fits
    assert _check(tg, 1, [[(0, 1, 4)], [(1, 1, 2)]], 2) == E_ARG                 # offset + length > L_w
    assert _check(tg, 1, [[(0, 0xFFFFFFFF, 2)], [(1, 1, 2)]], 2) == E_ARG        # (no 32-bit wrap-around)
    assert _check(tg, 1, ok, 1) == E_ARG                                         # keyword_id >= n_keywords
    assert _check(tg, 1, ok, 2, tgt_ptr=[0, 3, 2]) == E_ARG                      # tgt_ptr decreases
    assert _check(tg, 1, ok, 2, tgt_ptr=[1, 2, 3]) == E_ARG                      # tgt_ptr does not begin with 0
    assert _check(tg, 1, ok, 2, spell_off=[0, 5, 4]) == E_ARG                    # spell_off decreases
    assert _check(tg, 1, ok, 2, spell_off=[1, 4, 7]) == E_ARG                    # spell_off does not begin with 0
    assert _check(tg, 1, ok, 2, n_targets=1 << 31) == E_ARG                      # (checked before the arrays are read that far)
    assert _check([b"ab"], 0, [[(0, 0, 1)]], 1, tgt_ptr=[0, 1 << 31]) == E_ARG   # 2^31 terms (checked before terms[] is read)
    assert acm.lib().acm_approx_check(None, None, None, None, 0, 0) == E_ARG
    with pytest.raises(acm.ACMError):
        binding.ApproxSet(tg, 1, ok).check(1)
    binding.ApproxSet(tg, 1, ok).check(2)


def test_approx_split_is_the_canonical_cut():
    L = acm.lib()
    b, e = C.c_uint64(0), C.c_uint64(0)
    for length in (1, 2, 3, 7, 8, 15, 16, 17, 300, (1 << 31) - 1):
        for k in (0, 1, 2, 3, 7, 255):
            if length < k + 1:
                assert L.acm_approx_split(length, k, 0, C.byref(b), C.byref(e)) == E_ARG     # fewer symbols than pieces
                continue
            got = []
            for j in range(k + 1):
                assert L.acm_approx_split(length, k, j, C.byref(b), C.byref(e)) == 0
                got.append((b.value, e.value))
            assert got == split(length, k)
            assert got[0][0] == 0 and got[-1][1] == length and all(x[1] == y[0] for x, y in zip(got, got[1:])) and all(x[0] < x[1] for x in got)
            assert L.acm_approx_split(length, k, k + 1, C.byref(b), C.byref(e)) == E_ARG
    assert L.acm_approx_split(4, 3, 0, C.byref(b), C.byref(e)) == 0 and (b.value, e.value) == (0, 1)      # L == k + 1: pieces of one symbol
    assert L.acm_approx_split(3, 3, 0, C.byref(b), C.byref(e)) == E_ARG                                   # L < k + 1
    assert L.acm_approx_split(1 << 31, 0, 0, C.byref(b), C.byref(e)) == E_ARG
    assert L.acm_approx_split(4, 1, 0, None, C.byref(e)) == E_ARG
    with pytest.raises(ValueError):
        binding.ApproxSet.from_targets(acm.Machine(1), [b"abc"], 3)


def test_approx_records_equals_the_definition_and_the_hamming_scan_on_300_random_cases():
    rng = np.random.default_rng(1975)
    matches = inexact = many_seeds = cut_texts = ties = 0
    for trial in range(300):
        targets, ks, text, offsets = random_case(rng)
        kws, terms = compile_targets(targets, ks)
        rec = oracle_records([bytes(kw) for kw in kws], text)
        want = approx(rec, text, targets, ks, terms, offsets)
        same(want, hamming_scan(text, targets, ks, offsets), (trial, "the two derivations"))
        aset = binding.ApproxSet(targets, ks, terms)
        got = binding.approx_records(rec, aset, text, offsets=offsets, n_keywords=len(kws))
        same(got, want, (trial, targets, ks, text, offsets))
        if offsets.size == 2:                                                    # one text: offsets NULL says the same
            same(binding.approx_records(rec, aset, text, n_keywords=len(kws)), want, trial)
        matches += want[0].size
        inexact += int(np.count_nonzero(want[1]))
        many_seeds += int(np.count_nonzero(want[1] < np.asarray(ks, np.uint32)[want[0]["keyword_id"]]))   # d < k: at least two pieces are exact
        ties += int(np.count_nonzero(want[0]["end_pos"][1:] == want[0]["end_pos"][:-1]))
        cut_texts += offsets.size > 2
    print("matches %d, with mismatches %d, seeded more than once %d, ties in end_pos %d, trials with cuts %d" % (matches, inexact, many_seeds, ties, cut_texts))
    assert matches > 2000 and inexact > 1000 and many_seeds > 300 and ties > 100 and cut_texts > 100


def test_incomplete_term_sets_lose_matches_by_the_seed_condition():
    text = b"abcdefgh abcdeXgh abXdefgh Xbcdefgh abcdXfgh abXdeXgh"
    targets, ks = [b"abcdefgh"], [1]
    kws, full = compile_targets(targets, ks)
    assert full == [[(0, 0, 4), (1, 4, 4)]]
    rec = oracle_records([bytes(kw) for kw in kws], text)
    whole = approx(rec, text, targets, ks, full)
    same(whole, hamming_scan(text, targets, ks))
    assert whole[0].size == 5 and whole[1].tolist() == [0, 1, 1, 1, 1]
    # only the first piece: an occurrence whose mismatch lies in `abcd` has no seed
    first = [[(0, 0, 4)]]
    want = approx(rec, text, targets, ks, first)
    assert want[0]["end_pos"].tolist() == [7, 16, 43] and want[1].tolist() == [0, 1, 1]
    same(binding.approx_records(rec, binding.ApproxSet(targets, ks, first), text, n_keywords=2), want)
    # only the second piece; both pieces the other way round; one piece twice (emitted once)
    for terms in ([[(1, 4, 4)]], [[(1, 4, 4), (0, 0, 4)]], [[(0, 0, 4), (0, 0, 4)]], [[(1, 4, 4), (0, 0, 4), (1, 4, 4)]]):
        want = approx(rec, text, targets, ks, terms)
        assert 0 < want[0].size <= whole[0].size
        same(binding.approx_records(rec, binding.ApproxSet(targets, ks, terms), text, n_keywords=2), want, terms)
    # a term whose length is not its keyword's never seeds; a budget above the number of pieces still needs a seed
    assert binding.approx_records(rec, binding.ApproxSet(targets, ks, [[(0, 0, 3)]]), text, n_keywords=2)[0].size == 0
    want = approx(rec, text, targets, [3], full)
    assert want[0].size == 5 and hamming_scan(text, targets, [3])[0].size > 5    # `abXdeXgh` is within 3, and has no seed
    same(binding.approx_records(rec, binding.ApproxSet(targets, [3], full), text, n_keywords=2), want)


def test_counting_only_overflow_and_refused_records(novel_bytes):
    text = novel_bytes[:6000]
    targets, ks = [b"Clarissa", b"Dalloway", b"the"], [2, 1, 1]
    kws, terms = compile_targets(targets, ks)
    rec = oracle_records([bytes(kw) for kw in kws], text)
    want = approx(rec, text, targets, ks, terms)
    same(want, hamming_scan(text, targets, ks), "the two derivations")
    per = np.bincount(want[0]["keyword_id"], minlength=3)
    print("records %d, matches per target %s, with mismatches %d" % (rec.size, per.tolist(), int(np.count_nonzero(want[1]))))
    assert np.all(per > 0) and np.count_nonzero(want[1]) > 10
    aset = binding.ApproxSet(targets, ks, terms)
    same(binding.approx_records(rec, aset, text, n_keywords=len(kws)), want)
    L = acm.lib()
    t = np.frombuffer(text, np.uint8)
    n = C.c_uint64(0)
    total = want[0].size

    def call(out, dist, cap, records=rec, n_symbols=len(text), pos_base=0, off=None, n_texts=0, sym_bytes=1):
        return L.acm_approx_records(records.ctypes.data, records.size, t.ctypes.data, sym_bytes, n_symbols, pos_base,
                                    off.ctypes.data if off is not None else None, n_texts, *aset.args(), len(kws),
                                    out.ctypes.data if out is not None else None, dist.ctypes.data if dist is not None else None, cap, C.byref(n))
    assert call(None, None, 0) == 0 and n.value == total                         # count only
    out, dist = np.zeros(total, po.RECORD_DTYPE), np.full(total, 0x5555, np.uint32)
    out["end_pos"] = 0x5555
    n.value = 0
    assert call(out, dist, total - 1) == E_OVERFLOW and n.value == total and np.all(out["end_pos"] == 0x5555) and np.all(dist == 0x5555)
    assert call(out, None, total) == 0 and n.value == total and np.all(dist == 0x5555)     # dist may be NULL
    assert np.array_equal(out, want[0])
    assert call(out, dist, total) == 0
    same((out, dist), want)
    # nonzero pos_base
    shifted, moved = rec.copy(), want[0].copy()
    shifted["end_pos"] += 1 << 40
    moved["end_pos"] += 1 << 40
    same(approx(shifted, text, targets, ks, terms, pos_base=1 << 40), (moved, want[1]))
    same(binding.approx_records(shifted, aset, text, pos_base=1 << 40, n_keywords=len(kws)), (moved, want[1]))
    # records outside [pos_base, pos_base + n_symbols), their end or their start, or of length 0; offsets that break the contract
    assert call(out, dist, total, records=shifted) == E_ARG                      # ends behind the buffer
    assert call(out, dist, total, n_symbols=int(rec["end_pos"][-1])) == E_ARG    # the last record ends at n_symbols
    assert call(out, dist, total, pos_base=int(rec["end_pos"][0])) == E_ARG        # the first record ends at pos_base and begins in front of it
    zero = rec.copy()
    zero["length"][3] = 0
    assert call(out, dist, total, records=zero) == E_ARG
    assert call(out, dist, total, sym_bytes=0) == E_ARG
    for off in ([0, 10, 5, len(text)], [1, len(text)], [0, len(text) - 1]):
        assert call(out, dist, total, off=np.array(off, np.uint64), n_texts=len(off) - 1) == E_ARG
    same((out, dist), want)                                                      # nothing was written by the refused calls


def test_wider_symbols_compare_all_their_bytes():
    high = 0x4100000000000000
    for sb, dt in ((2, np.uint16), (4, np.uint32), (8, np.uint64)):
        hi = high >> (64 - 8 * sb)
        text = (np.frombuffer(b"abcdefgh abcdeXgh", np.uint8).astype(np.uint64) | np.uint64(hi)).astype(dt)
        text[3] ^= dt(hi)                                                        # `d` with another high byte: a mismatch no low-byte compare sees
        target = (np.frombuffer(b"abcdefgh", np.uint8).astype(np.uint64) | np.uint64(hi)).astype(dt)
        kws, terms = compile_targets([target], [1])
        rec = brute(kws, text)
        want = approx(rec, text, [target], [1], terms)
        same(want, hamming_scan(text, [target], [1]))
        assert want[1].tolist() == [1, 1]
        same(binding.approx_records(rec, binding.ApproxSet([target], [1], terms), text, n_keywords=len(kws)), want, sb)


def test_from_targets_cuts_canonically_and_reuses_ids():
    m = acm.Machine(1)
    m.add_keyword(b"efgh")
    targets, ks = [b"abcdefgh", b"abcdxyz", b"ab"], [1, 2, 0]
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    kws, terms = compile_targets(targets, ks, keywords=[tuple(b"efgh")])
    assert [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws and aset.n_keywords == len(kws) == 5
    assert aset.terms.tolist() == [list(t) for p in terms for t in p] and aset.tgt_ptr.tolist() == [0, 2, 5, 6]
    assert aset.spell_off.tolist() == [0, 8, 15, 17] and aset.k.tolist() == ks and bytes(aset.spell_data) == b"".join(targets)
    assert binding.ApproxSet.from_targets(m, [b"abcdefgh"], 1).terms.tolist() == [[1, 0, 4], [0, 4, 4]] and m.nb_keywords == 5   # a scalar k; nothing new
    m4 = acm.Machine(4)
    a4 = binding.ApproxSet.from_targets(m4, [np.array([70000, 70001, 5, 70000], np.uint32)], 1)
    assert a4.sym_size == 4 and a4.terms.tolist() == [[0, 0, 2], [1, 2, 2]] and a4.spell_data.dtype == np.uint32


def _scan_approx(h, text, aset, cap, offsets=None, sym_bytes=1):
    L = acm.lib()
    out, dist = np.zeros(max(cap, 1), po.RECORD_DTYPE), np.zeros(max(cap, 1), np.uint32)
    n = C.c_uint64(0)
    off = np.ascontiguousarray(offsets, np.uint64) if offsets is not None else None
    rc = L.acm_scan_approx(h, text.ctypes.data if text.size else None, text.size, off.ctypes.data if off is not None else None,
                           off.size - 1 if off is not None else 0, *aset.args(), out.ctypes.data if cap else None, dist.ctypes.data, cap, C.byref(n))
    return rc, int(n.value), (out[:min(int(n.value), cap)], dist[:min(int(n.value), cap)])


def test_acm_scan_approx_on_a_case_insensitive_machine_takes_the_host_loop(kat):
    cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
    m = acm.Machine(1, cmp=cmp)
    targets, ks = [b"clarissa", b"dalloway"], [2, 1]
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    text = b"Clarissa CLARISSE Dalloway DALLOWAX clarixxa dallowxx clarisXXX cLaRiSsA"
    t = np.frombuffer(text, np.uint8)
    assert acm.lib().acm_scan_approx(m.handle, t.ctypes.data, t.size, None, 0, *aset.args(), None, None, 0, C.byref(C.c_uint64(0))) == E_INELIGIBLE
    m.set_symbol_bytes(1)                                                        # (the host loop needs the symbol size)
    want = hamming_scan(text.lower(), targets, ks)                               # symbols compare as the machine compares them
    assert want[0].size == 7 and want[1].tolist() == [0, 1, 0, 1, 2, 2, 0]     # (`clarisXX` of clarisXXX is within 2 as well)
    assert hamming_scan(text, targets, ks)[0].size < want[0].size                # (the exact-case reading finds fewer)
    kws, terms = compile_targets(targets, ks)
    same(approx(oracle_records([bytes(kw) for kw in kws], text.lower()), text.lower(), targets, ks, terms), want, "the two derivations")
    rc, n, got = _scan_approx(m.handle, t, aset, want[0].size)
    assert rc == 0 and m.scan_path == PATH_LOOP
    same(got, want)
    same(m.scan_approx(text, aset), want)
    rc, n, got = _scan_approx(m.handle, t, aset, want[0].size - 1)               # too little room: the count that suffices
    assert rc == E_OVERFLOW and n == want[0].size
    rc, n, got = _scan_approx(m.handle, t, aset, 0)                              # no room at all only counts
    assert rc == 0 and n == want[0].size
    # a batch: a cut inside `Dalloway`
    offsets = np.array([0, 0, 9, 21, len(text)], np.uint64)
    cut = hamming_scan(text.lower(), targets, ks, offsets)
    assert 0 < cut[0].size < want[0].size
    same(_scan_approx(m.handle, t, aset, want[0].size, offsets=offsets)[2], cut)
    assert _scan_approx(m.handle, t[:0], aset, 4)[:2] == (0, 0)
    # this call knows the machine: a term whose length or spelling is not its keyword's piece is an argument error
    wrong = binding.ApproxSet(targets, ks, [[(0, 0, 3), (1, 2, 3), (2, 5, 3)], [(3, 0, 4), (4, 4, 4)]])
    assert _scan_approx(m.handle, t, wrong, 8)[0] == E_ARG
    moved = binding.ApproxSet(targets, ks, [[(0, 1, 2), (1, 2, 3), (2, 5, 3)], [(3, 0, 4), (4, 4, 4)]])   # `cl` is not spelled at offset 1
    assert _scan_approx(m.handle, t, moved, 8)[0] == E_ARG
    folded = binding.ApproxSet([b"CLARISSA", b"dalloway"], ks, [list(map(tuple, aset.terms[:3])), list(map(tuple, aset.terms[3:]))])
    assert _scan_approx(m.handle, t, folded, 8)[0] == 0                          # (spelled as the machine compares)
    assert _scan_approx(m.handle, t, aset, 8, offsets=[0, 7, 5, len(text)])[0] == E_ARG
