"""Keywords within edit distance k on the host (acm_edit_check, acm_edit_records, the host path of acm_scan_edit).
The expected answer is always the definition of EDIT in Python over the ORACLE's or tests/brute.py's records
(tests/edit_cases.py: a free-start Sellers pass with the largest-start rule, then the seed condition) and, for
canonical cuts, a second derivation from the text alone (a plain Levenshtein distance for every end and start) --
never the library's own scan or verification.  All comparisons are exact, order, lengths and distances included.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.approx_cases import brute, compile_targets, oracle_records, same
from tests.edit_cases import ed, edit_scan, edits, seeds_of

E_ARG, E_OVERFLOW, E_INELIGIBLE = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, binding.ACM_GPU_E_INELIGIBLE
PATH_LOOP = 3


def _checks(targets, k, terms, n_keywords, spell_off=None, tgt_ptr=None, n_targets=None):
    """(acm_edit_check, acm_approx_check) on lists, or on raw arrays"""
    a = binding.ApproxSet(targets, k, terms)
    so = a.spell_off if spell_off is None else np.asarray(spell_off, np.uint64)
    tp = a.tgt_ptr if tgt_ptr is None else np.asarray(tgt_ptr, np.uint64)
    n = a.n_targets if n_targets is None else n_targets
    args = (so.ctypes.data, a.k.ctypes.data if a.k.size else None, a.terms.ctypes.data if a.terms.size else None, tp.ctypes.data, n, n_keywords)
    return acm.lib().acm_edit_check(*args), acm.lib().acm_approx_check(*args)


def test_edit_check_names_every_argument_error_of_approx_check_and_its_own_two():
    tg, ok = [b"abcd", b"xyz"], [[(0, 0, 2), (1, 2, 2)], [(1, 1, 2)]]
    assert _checks(tg, 1, ok, 2) == (0, 0)
    assert _checks([], 0, [], 0) == (0, 0)                                           # no target is a set
    both = [dict(tgt_ptr=[0, 2, 2]), dict(spell_off=[0, 4, 4]), dict(spell_off=[0, 1 << 31, (1 << 31) + 3]), dict(tgt_ptr=[0, 3, 2]),
            dict(tgt_ptr=[1, 2, 3]), dict(spell_off=[0, 5, 4]), dict(spell_off=[1, 4, 7]), dict(n_targets=1 << 31)]
    for raw in both:                                                                 # acm_approx_check's errors on raw arrays
        assert _checks(tg, 1, ok, 2, **raw) == (E_ARG, E_ARG), raw
    assert _checks(tg, [1, 256], ok, 2) == (E_ARG, E_ARG)                            # k > 255
    assert _checks(tg, 1, [[(0, 0, 0)], [(1, 1, 2)]], 2) == (E_ARG, E_ARG)           # length 0
    assert _checks(tg, 1, [[(0, 0, 4)], [(1, 1, 2)]], 2) == (0, 0)                   # offset + length == L_w: the last that fits
    assert _checks(tg, 1, [[(0, 1, 4)], [(1, 1, 2)]], 2) == (E_ARG, E_ARG)           # offset + length > L_w
    assert _checks(tg, 1, [[(0, 0xFFFFFFFF, 2)], [(1, 1, 2)]], 2) == (E_ARG, E_ARG)  # (no 32-bit wrap-around)
    assert _checks(tg, 1, ok, 1) == (E_ARG, E_ARG)                                   # keyword_id >= n_keywords
    assert _checks([b"ab"], 0, [[(0, 0, 1)]], 1, tgt_ptr=[0, 1 << 31]) == (E_ARG, E_ARG)   # 2^31 terms
    assert acm.lib().acm_edit_check(None, None, None, None, 0, 0) == E_ARG
    # the two conditions of the edit calls: the same arguments pass acm_approx_check
    long = [b"a" * 40, b"xyz"]
    assert _checks(long, [15, 1], ok, 2) == (0, 0)
    assert _checks(long, [16, 1], ok, 2) == (E_ARG, 0)                               # k = 16
    assert _checks(long, [255, 1], ok, 2) == (E_ARG, 0)
    assert _checks(tg, [3, 2], ok, 2) == (0, 0)                                      # k = L - 1
    assert _checks(tg, [4, 1], ok, 2) == (E_ARG, 0)                                  # k = L
    assert _checks(tg, [1, 3], ok, 2) == (E_ARG, 0)                                  # k = L of the second target
    assert _checks(tg, [1, 7], ok, 2) == (E_ARG, 0)                                  # k > L
    with pytest.raises(acm.ACMError):
        binding.ApproxSet(tg, [4, 1], ok).check_edit(2)
    binding.ApproxSet(tg, [4, 1], ok).check(2)
    binding.ApproxSet(tg, [3, 2], ok).check_edit(2)
    binding.ApproxSet(tg, [3, 2], ok).check_edit()                                   # (the set's own number of keywords)


def _random_case(rng):
    """(targets, ks, text, offsets): 1 to 3 targets of 2 to 10 symbols over {a, b} or {a, b, c} with k of 0 to 3 (below
    the target's length), a text of 0 to 60 symbols cut into 1 to 4 texts, empty ones included"""
    alphabet = np.frombuffer(b"ab" if rng.integers(0, 2) else b"abc", np.uint8)
    targets, ks = [], []
    for _ in range(int(rng.integers(1, 4))):
        L = int(rng.integers(2, 11))
        targets.append(bytes(rng.choice(alphabet, size=L)))
        ks.append(int(rng.integers(0, min(4, L))))
    n = int(rng.integers(0, 61))
    text = bytes(rng.choice(alphabet, size=n))
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 4))))
    return targets, ks, text, np.array([0] + [int(c) for c in cuts] + [n], np.uint64)


def test_edit_records_equals_both_derivations_on_300_random_cases():
    rng = np.random.default_rng(1975)
    matches = shorter = equal = longer = many_seeds = cut_texts = empty_texts = 0
    by_dist = [0, 0, 0, 0]
    for trial in range(300):
        targets, ks, text, offsets = _random_case(rng)
        kws, terms = compile_targets(targets, ks)
        rec = oracle_records([bytes(kw) for kw in kws], text)
        want = edits(rec, text, targets, ks, terms, offsets)
        same(want, edit_scan(text, targets, ks, offsets), (trial, "the two derivations", targets, ks, text, offsets))
        aset = binding.ApproxSet(targets, ks, terms)
        got = binding.edit_records(rec, aset, text, offsets=offsets, n_keywords=len(kws))
        same(got, want, (trial, targets, ks, text, offsets))
        if offsets.size == 2:                                                        # one text: offsets NULL says the same
            same(binding.edit_records(rec, aset, text, n_keywords=len(kws)), want, trial)
        L_of = np.array([len(t) for t in targets], np.uint32)[want[0]["keyword_id"]]
        matches += want[0].size
        shorter += int(np.count_nonzero(want[0]["length"] < L_of))
        equal += int(np.count_nonzero(want[0]["length"] == L_of))
        longer += int(np.count_nonzero(want[0]["length"] > L_of))
        for d in range(4):
            by_dist[d] += int(np.count_nonzero(want[1] == d))
        off = [int(x) for x in offsets]
        for r in want[0][:3]:                                                        # (a few per trial: the count is a Python loop)
            e, w = int(r["end_pos"]), int(r["keyword_id"])
            t = max(i for i in range(len(off) - 1) if off[i] <= e)
            many_seeds += seeds_of(rec, (off[t], off[t + 1]), e, len(targets[w]), ks[w], terms[w]) >= 3
        cut_texts += offsets.size > 2
        empty_texts += bool(np.any(offsets[1:] == offsets[:-1]))
    print("matches %d: shorter / equal / longer than the target %d / %d / %d, by distance %s, of those looked at reached from >= 3 seeds %d; "
          "trials with cuts %d, with empty texts %d" % (matches, shorter, equal, longer, by_dist, many_seeds, cut_texts, empty_texts))
    assert matches > 2000 and shorter > 200 and equal > 200 and longer > 50
    assert all(n > 100 for n in by_dist) and many_seeds > 50 and cut_texts > 100 and empty_texts > 20


def _one(target, k, text, offsets=None, terms=None):
    """(got, want, records) of one byte target with the canonical cut (or `terms`) over a byte text; the two derivations agree"""
    kws, cut = compile_targets([target], [k])
    rec = oracle_records([bytes(kw) for kw in kws], text)
    want = edits(rec, text, [target], [k], cut if terms is None else terms, offsets)
    if terms is None:
        same(want, edit_scan(text, [target], [k], offsets), ("the two derivations", target, k, text))
    aset = binding.ApproxSet([target], [k], cut if terms is None else terms)
    got = binding.edit_records(rec, aset, text, offsets=offsets, n_keywords=len(kws))
    same(got, want, (target, k, text, offsets))
    return got, want, rec


def test_named_small_cases():
    # one deletion, one insertion, one substitution; at the first, a middle and the last symbol
    for word, kind in ((b"Daloway", "deletion"), (b"Dallloway", "insertion"), (b"Dalloxay", "substitution"), (b"alloway", "first"), (b"Dallowa", "last"),
                       (b"Xalloway", "first"), (b"DallowaX", "last"), (b"XDalloway", "first"), (b"DallowayX", "last")):
        assert ed(list(b"Dalloway"), list(word)) == 1, word
        text = b"Mrs " + word + b" said"
        got, want, _ = _one(b"Dalloway", 1, text)
        best = [(int(r["end_pos"]), int(r["length"]), int(d)) for r, d in zip(*got) if d == min(got[1])]
        assert got[0].size >= 1 and min(got[1]) <= 1, (word, kind)
        if word in (b"Daloway", b"Dallloway", b"Dalloxay"):
            assert (4 + len(word) - 1, len(word), 1) in best, (word, best)          # the word itself is the shortest best match at its end
    assert _one(b"Dalloway", 1, b"Mrs Daloway said")[0][0].size >= 1                # (the issue's own example: APPROX never reports it)
    # a transposition costs 2
    assert ed(list(b"Dalloway"), list(b"Dalolway")) == 2
    assert _one(b"Dalloway", 1, b"Mrs Dalolway said")[0][0].size == 0
    got = _one(b"Dalloway", 2, b"Mrs Dalolway said")[0]
    assert 2 in got[1].tolist() and min(got[1]) == 2
    # a periodic text: many seeds reach each end
    got, want, rec = _one(b"abab", 1, b"abababab")
    kws, terms = compile_targets([b"abab"], [1])
    assert terms == [[(0, 0, 2), (0, 2, 2)]]                                         # two identical pieces: two terms share one keyword
    assert max(seeds_of(rec, (0, 8), int(r["end_pos"]), 4, 1, terms[0]) for r in got[0]) >= 3
    assert got[0]["end_pos"].tolist() == [2, 3, 4, 5, 6, 7] and got[1].tolist() == [1, 0, 1, 0, 1, 0]   # every end from `aba` on; exact at 3, 5, 7
    _one(b"abab", 1, b"xxababxx")
    _one(b"abab", 1, b"ab")
    # a text that ends inside a target, and one that begins inside it
    got = _one(b"Dalloway", 2, b"said Dallow")[0]
    assert got[0].size >= 1 and int(got[0]["end_pos"][-1]) == 10 and int(got[1][-1]) == 2
    got = _one(b"Dalloway", 2, b"lloway said")[0]
    assert got[0].size >= 1 and (5, 6, 2) in [(int(r["end_pos"]), int(r["length"]), int(d)) for r, d in zip(*got)]
    got = _one(b"Dalloway", 2, b"Mrs Dalloway said", offsets=np.array([0, 8, 17], np.uint64))[0]     # a cut inside the word: both halves are too far
    assert got[0].size == 0
    got = _one(b"Dalloway", 3, b"Mrs Dalloway said", offsets=np.array([0, 9, 9, 17], np.uint64))[0]  # `Dallo` | `way said`: `Dallo` is within 3
    assert got[0].size >= 1 and all(int(e) < 9 for e in got[0]["end_pos"])
    # k = 0 equals the exact occurrences
    text = b"the cat sat on the mat; the end"
    got = _one(b"the", 0, text)[0]
    assert got[0]["end_pos"].tolist() == [i + 2 for i in range(len(text)) if text[i:i + 3] == b"the"] and set(got[0]["length"].tolist()) == {3}
    assert got[1].tolist() == [0, 0, 0]


def test_incomplete_term_sets_lose_matches_by_the_seed_condition():
    text = b"abcdefgh abcdeXgh abXdefgh bcdefgh abcdfgh abXdeXgh abcdefg"
    target, k = b"abcdefgh", 1
    kws, full = compile_targets([target], [k])
    assert full == [[(0, 0, 4), (1, 4, 4)]]
    whole = _one(target, k, text)[0]
    assert whole[0].size > 6
    for terms in ([[(0, 0, 4)]], [[(1, 4, 4)]], [[(1, 4, 4), (0, 0, 4)]], [[(0, 0, 4), (0, 0, 4)]], [[(1, 4, 4), (0, 0, 4), (1, 4, 4)]]):
        got = _one(target, k, text, terms=terms)[0]
        assert 0 < got[0].size <= whole[0].size, terms
    assert _one(target, k, text, terms=[[(0, 0, 4)]])[0][0].size < whole[0].size     # an edit inside `abcd` leaves no seed
    assert _one(target, k, text, terms=[[(0, 0, 3)]])[0][0].size == 0                # a term whose length is not its keyword's never seeds
    rec = oracle_records([bytes(kw) for kw in kws], text)
    wide = edits(rec, text, [target], [3], full)                                     # a budget above the number of pieces still needs a seed
    assert wide[0].size < edit_scan(text, [target], [3])[0].size
    same(binding.edit_records(rec, binding.ApproxSet([target], [3], full), text, n_keywords=2), wide)


def test_counting_only_overflow_and_refused_records(novel_bytes):
    text = novel_bytes[:3000]
    targets, ks = [b"Clarissa", b"Dalloway", b"the"], [2, 1, 1]
    kws, terms = compile_targets(targets, ks)
    rec = oracle_records([bytes(kw) for kw in kws], text)
    want = edits(rec, text, targets, ks, terms)
    per = np.bincount(want[0]["keyword_id"], minlength=3)
    print("records %d, matches per target %s, with edits %d" % (rec.size, per.tolist(), int(np.count_nonzero(want[1]))))
    assert np.all(per > 0) and np.count_nonzero(want[1]) > 10
    aset = binding.ApproxSet(targets, ks, terms)
    same(binding.edit_records(rec, aset, text, n_keywords=len(kws)), want)
    L = acm.lib()
    t = np.frombuffer(text, np.uint8)
    n = C.c_uint64(0)
    total = want[0].size

    def call(out, dist, cap, records=rec, n_symbols=len(text), pos_base=0, off=None, n_texts=0, sym_bytes=1, a=aset):
        return L.acm_edit_records(records.ctypes.data, records.size, t.ctypes.data, sym_bytes, n_symbols, pos_base,
                                  off.ctypes.data if off is not None else None, n_texts, *a.args(), len(kws),
                                  out.ctypes.data if out is not None else None, dist.ctypes.data if dist is not None else None, cap, C.byref(n))
    assert call(None, None, 0) == 0 and n.value == total                             # count only
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
    same(edits(shifted, text, targets, ks, terms, pos_base=1 << 40), (moved, want[1]))
    same(binding.edit_records(shifted, aset, text, pos_base=1 << 40, n_keywords=len(kws)), (moved, want[1]))
    # refused: records outside the buffer or of length 0, offsets that break the contract, a set the edit calls do not take
    assert call(out, dist, total, records=shifted) == E_ARG
    assert call(out, dist, total, n_symbols=int(rec["end_pos"][-1])) == E_ARG
    assert call(out, dist, total, pos_base=int(rec["end_pos"][0])) == E_ARG
    zero = rec.copy()
    zero["length"][3] = 0
    assert call(out, dist, total, records=zero) == E_ARG
    assert call(out, dist, total, sym_bytes=0) == E_ARG
    for off in ([0, 10, 5, len(text)], [1, len(text)], [0, len(text) - 1]):
        assert call(out, dist, total, off=np.array(off, np.uint64), n_texts=len(off) - 1) == E_ARG
    assert call(out, dist, total, a=binding.ApproxSet(targets, [2, 1, 3], terms)) == E_ARG   # k = L
    same((out, dist), want)                                                          # nothing was written by the refused calls


def test_wider_symbols_compare_all_their_bytes():
    high = 0x4100000000000000
    for sb, dt in ((2, np.uint16), (4, np.uint32), (8, np.uint64)):
        hi = high >> (64 - 8 * sb)
        text = (np.frombuffer(b"abcdefgh abcdeXgh abcefgh", np.uint8).astype(np.uint64) | np.uint64(hi)).astype(dt)
        text[3] ^= dt(hi)                                                            # `d` with another high byte: an edit no low-byte compare sees
        target = (np.frombuffer(b"abcdefgh", np.uint8).astype(np.uint64) | np.uint64(hi)).astype(dt)
        kws, terms = compile_targets([target], [1])
        rec = brute(kws, text)
        want = edits(rec, text, [target], [1], terms)
        same(want, edit_scan(text, [target], [1]))
        assert (7, 8, 0, 1) in [(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"]), int(d)) for r, d in zip(*want)]
        assert 0 not in want[1].tolist()                                             # (a low-byte compare would find `abcdefgh` exactly)
        same(binding.edit_records(rec, binding.ApproxSet([target], [1], terms), text, n_keywords=len(kws)), want, sb)


def _scan_edit(h, text, aset, cap, offsets=None):
    L = acm.lib()
    out, dist = np.zeros(max(cap, 1), po.RECORD_DTYPE), np.zeros(max(cap, 1), np.uint32)
    n = C.c_uint64(0)
    off = np.ascontiguousarray(offsets, np.uint64) if offsets is not None else None
    rc = L.acm_scan_edit(h, text.ctypes.data if text.size else None, text.size, off.ctypes.data if off is not None else None,
                         off.size - 1 if off is not None else 0, *aset.args(), out.ctypes.data if cap else None, dist.ctypes.data, cap, C.byref(n))
    return rc, int(n.value), (out[:min(int(n.value), cap)], dist[:min(int(n.value), cap)])


def test_acm_scan_edit_on_a_case_insensitive_machine_takes_the_host_loop(kat):
    cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
    m = acm.Machine(1, cmp=cmp)
    targets, ks = [b"clarissa", b"dalloway"], [2, 1]
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    text = b"Clarissa CLARISE Daloway DALLLOWAY clarixxa dallowxx clarisXXX cLaRiSsA"
    t = np.frombuffer(text, np.uint8)
    assert acm.lib().acm_scan_edit(m.handle, t.ctypes.data, t.size, None, 0, *aset.args(), None, None, 0, C.byref(C.c_uint64(0))) == E_INELIGIBLE
    m.set_symbol_bytes(1)                                                            # (the host loop needs the symbol size)
    want = edit_scan(text.lower(), targets, ks)                                      # symbols compare as the machine compares them
    assert edit_scan(text, targets, ks)[0].size < want[0].size                       # (the exact-case reading finds fewer)
    kws, terms = compile_targets(targets, ks)
    same(edits(oracle_records([bytes(kw) for kw in kws], text.lower()), text.lower(), targets, ks, terms), want, "the two derivations")
    ends = want[0]["end_pos"].tolist()
    assert 7 in ends and 15 in ends and 23 in ends and 33 in ends and len(text) - 1 in ends     # the deletion and the insertion are found
    rc, n, got = _scan_edit(m.handle, t, aset, want[0].size)
    assert rc == 0 and m.scan_path == PATH_LOOP
    same(got, want)
    same(m.scan_edit(text, aset), want)
    rc, n, got = _scan_edit(m.handle, t, aset, want[0].size - 1)                     # too little room: the count that suffices
    assert rc == E_OVERFLOW and n == want[0].size
    rc, n, got = _scan_edit(m.handle, t, aset, 0)                                    # no room at all only counts
    assert rc == 0 and n == want[0].size
    offsets = np.array([0, 0, 9, 21, len(text)], np.uint64)                          # a batch: a cut inside `Daloway`
    cut = edit_scan(text.lower(), targets, ks, offsets)
    assert 0 < cut[0].size < want[0].size
    same(_scan_edit(m.handle, t, aset, want[0].size, offsets=offsets)[2], cut)
    assert _scan_edit(m.handle, t[:0], aset, 4)[:2] == (0, 0)
    # this call knows the machine, and adds the two conditions
    wrong = binding.ApproxSet(targets, ks, [[(0, 0, 3), (1, 2, 3), (2, 5, 3)], [(3, 0, 4), (4, 4, 4)]])
    assert _scan_edit(m.handle, t, wrong, 8)[0] == E_ARG
    budget = binding.ApproxSet(targets, [8, 1], [list(map(tuple, aset.terms[:3])), list(map(tuple, aset.terms[3:]))])
    assert _scan_edit(m.handle, t, budget, 8)[0] == E_ARG                            # k = L
    assert _scan_edit(m.handle, t, aset, 8, offsets=[0, 7, 5, len(text)])[0] == E_ARG
