"""Keyword templates with symbol classes on the host (acm_templates_check, acm_templates_split,
acm_templates_records, the host path of acm_scan_templates, TemplateSet, template(), hex_template(), IUPAC).  The
expected answer is always tests/template_cases.py: the definition of TEMPLATES in plain Python over the oracle's
records, a window scan from the text alone, the canonical cut in plain Python and, for byte templates, Python's
`re` -- never the library's own scan or pass.  All comparisons are exact, order and distances included.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import ANY, IUPAC, SymbolClass, TemplateSet, hex_template, template
from oracle import pyoracle as po
from tests import template_cases as tc
from tests.template_cases import same

E_ARG, E_OVERFLOW, E_INELIGIBLE = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, binding.ACM_GPU_E_INELIGIBLE
LIT, ANYW = binding.ACM_TEMPLATE_LITERAL, binding.ACM_TEMPLATE_ANY
PATH_LOOP = 3
AB = SymbolClass([(97, 98)])
DIGIT = SymbolClass([(48, 57)])


def _check(tset, n_keywords, sym_bytes=1, **over):
    """acm_templates_check on a TemplateSet with some members of its spec replaced (arrays, or numbers)"""
    keep = []
    spec = binding.TemplateSpec.from_buffer_copy(tset.spec)
    for name, value in over.items():
        if isinstance(value, (list, np.ndarray)):
            dt = {"spell_off": np.uint64, "tgt_ptr": np.uint64, "cls_ptr": np.uint64, "ranges": np.uint8}.get(name, np.uint32)
            keep.append(np.ascontiguousarray(value, dtype=dt))
            value = keep[-1].ctypes.data
        setattr(spec, name, value)
    return acm.lib().acm_templates_check(C.byref(spec), sym_bytes, n_keywords)


def test_templates_check_names_every_argument_error():
    tpls = [[97, 98, AB, 100], [120, ANY, 122, DIGIT]]
    ok = [[(0, 0, 2)], [(1, 2, 1)]]
    good = TemplateSet(tpls, 1, ok)
    assert good.cells.tolist() == [LIT, LIT, 0, LIT, LIT, ANYW, LIT, 1] and good.cls_ptr.tolist() == [0, 1, 2]
    assert _check(good, 2) == 0
    assert _check(TemplateSet([], 0, []), 0) == 0                                # no template is a set
    # everything acm_approx_check refuses
    assert _check(good, 2, tgt_ptr=[0, 1, 1]) == E_ARG                           # a template without terms
    assert _check(good, 2, spell_off=[0, 4, 4]) == E_ARG                         # L_w == 0
    assert _check(TemplateSet(tpls, [1, 256], ok), 2) == E_ARG                   # k > 255
    assert _check(TemplateSet(tpls, [1, 255], ok), 2) == 0
    assert _check(TemplateSet(tpls, 1, [[(0, 0, 0)], [(1, 2, 1)]]), 2) == E_ARG  # length 0
    assert _check(TemplateSet(tpls, 1, [[(0, 3, 2)], [(1, 2, 1)]]), 2) == E_ARG  # offset + length > L_w
    assert _check(good, 1) == E_ARG                                              # keyword_id >= n_keywords
    assert _check(good, 2, tgt_ptr=[1, 1, 2]) == E_ARG                           # tgt_ptr does not begin with 0
    assert _check(good, 2, spell_off=[0, 5, 4]) == E_ARG                         # spell_off decreases
    assert _check(good, 2, n_templates=1 << 31) == E_ARG
    # cells
    assert _check(good, 2, cells=[LIT, LIT, 2, LIT, LIT, ANYW, LIT, 1]) == E_ARG            # a class id that is no class
    assert _check(good, 2, cells=[LIT, LIT, 0xFFFFFFFD, LIT, LIT, ANYW, LIT, 1]) == E_ARG   # neither constant nor a class id
    assert _check(TemplateSet(tpls, 1, [[(0, 1, 2)], [(1, 2, 1)]]), 2) == E_ARG  # a term over a class cell
    assert _check(TemplateSet(tpls, 1, [[(0, 0, 2)], [(1, 0, 2)]]), 2) == E_ARG  # a term over an ANY cell
    assert _check(TemplateSet(tpls, 1, [[(0, 3, 1)], [(1, 2, 1)]]), 2) == 0      # a term on the literal behind the class
    assert _check(good, 2, cells=None) == E_ARG
    # classes
    assert _check(good, 2, ranges=[98, 97, 48, 57]) == E_ARG                     # lo > hi
    assert _check(good, 2, ranges=[97, 97, 48, 57]) == 0                         # lo == hi
    assert _check(good, 2, cls_ptr=[0, 2, 1]) == E_ARG                           # cls_ptr decreases
    assert _check(good, 2, cls_ptr=[1, 1, 2]) == E_ARG                           # cls_ptr does not begin with 0
    assert _check(good, 2, n_classes=0xFFFFFFFE) == E_ARG
    assert _check(good, 2, cls_flags=None) == E_ARG
    assert _check(TemplateSet([[97, SymbolClass(range(0, 32, 2))]], 0, [[(0, 0, 1)]]), 1) == 0        # 16 ranges: the most
    assert _check(TemplateSet([[97, SymbolClass(range(0, 34, 2))]], 0, [[(0, 0, 1)]]), 1) == E_ARG    # 17 ranges
    assert _check(TemplateSet([[97, SymbolClass([])], [97, SymbolClass([], negate=True)]], 0, [[(0, 0, 1)], [(0, 0, 1)]]), 1) == 0   # empty classes
    for sb in (0, 3, 16):
        assert _check(good, 2, sym_bytes=sb) == E_ARG
    assert acm.lib().acm_templates_check(None, 1, 0) == E_ARG
    with pytest.raises(acm.ACMError):
        good.check(1)
    good.check(2)


def test_equal_classes_share_an_id():
    t = TemplateSet([[97, SymbolClass([(48, 57)]), DIGIT, AB, SymbolClass([(48, 57)], negate=True)]], 0, [[(0, 0, 1)]])
    assert t.cells.tolist() == [LIT, 0, 0, 1, 2] and t.cls_flags.tolist() == [0, 0, 1] and t.ranges.tolist() == [48, 57, 97, 98, 48, 57]


def _cells_of_runs(runs):
    """literal runs of the given lengths with one class cell between neighbours and around them"""
    cells = [AB]
    for n in runs:
        cells += [120] * n + [AB]
    return cells


def test_templates_split_is_the_canonical_cut():
    L = acm.lib()
    o, n = C.c_uint64(0), C.c_uint64(0)

    def got(cells, k):
        words = np.array([LIT if tc.is_literal(c) else ANYW if c is ANY else 0 for c in cells], np.uint32)
        out = []
        for j in range(k + 1):
            if L.acm_templates_split(words.ctypes.data, words.size, k, j, C.byref(o), C.byref(n)):
                return None
            out.append((o.value, n.value))
        assert L.acm_templates_split(words.ctypes.data, words.size, k, k + 1, C.byref(o), C.byref(n)) == E_ARG
        return out
    lengths = set()
    for runs in ([5], [2, 2], [3, 1, 3], [1, 1, 1], [7, 2], [300]):
        cells = _cells_of_runs(runs)
        for k in range(0, 3):
            want = tc.split(cells, k)
            assert got(cells, k) == want and want is not None, (runs, k)
            assert TemplateSet.split(cells, k) == want
            assert all(all(tc.is_literal(c) for c in cells[b:b + q]) for b, q in want) and all(x[0] + x[1] <= y[0] for x, y in zip(want, want[1:]))
            lengths.add((tuple(runs), k, want[0][1]))
    assert {((5,), 0, 5), ((5,), 1, 2), ((5,), 2, 1), ((2, 2), 0, 2), ((2, 2), 1, 2), ((2, 2), 2, 1), ((3, 1, 3), 0, 3), ((3, 1, 3), 1, 3),
            ((3, 1, 3), 2, 1), ((1, 1, 1), 2, 1)} <= lengths                     # q changes with the layout and with k
    assert tc.split(_cells_of_runs([3, 1, 3]), 0) == [(1, 3)]                    # k = 0: the first of the longest runs, whole
    assert tc.split(_cells_of_runs([2, 5, 5]), 0) == [(4, 5)] == got(_cells_of_runs([2, 5, 5]), 0)
    # one literal cell too few
    for runs, k in (([1, 1], 2), ([3], 3), ([], 0)):
        assert tc.split(_cells_of_runs(runs), k) is None and got(_cells_of_runs(runs), k) is None
        with pytest.raises(ValueError):
            TemplateSet.from_templates(acm.Machine(1), [_cells_of_runs(runs)], k)
    words = np.full(4, LIT, np.uint32)
    assert L.acm_templates_split(None, 4, 0, 0, C.byref(o), C.byref(n)) == E_ARG
    assert L.acm_templates_split(words.ctypes.data, 4, 0, 0, None, C.byref(n)) == E_ARG
    assert L.acm_templates_split(words.ctypes.data, 0, 0, 0, C.byref(o), C.byref(n)) == E_ARG


def test_templates_records_equals_the_definition_and_the_window_scan_on_200_random_cases():
    rng = np.random.default_rng(1975)
    matches = inexact = many_seeds = cut_texts = ties = by_class = 0
    for trial in range(200):
        tpls, ks, text, offsets = tc.random_case(rng)
        kws, terms = tc.compile_templates(tpls, ks)
        rec = tc.oracle_records([bytes(kw) for kw in kws], text)
        want = tc.templates(rec, text, tpls, ks, terms, offsets)
        same(want, tc.window_scan(text, tpls, ks, offsets), (trial, "the two derivations"))
        tset = TemplateSet(tpls, ks, terms)
        got = binding.templates_records(rec, tset, text, offsets=offsets, n_keywords=len(kws))
        same(got, want, (trial, tpls, ks, text, offsets))
        if offsets.size == 2:                                                    # one text: offsets NULL says the same
            same(binding.templates_records(rec, tset, text, n_keywords=len(kws)), want, trial)
        matches += want[0].size
        inexact += int(np.count_nonzero(want[1]))
        many_seeds += sum(tc.seeds_of(rec, terms, int(r["end_pos"]) + 1 - int(r["length"]), int(r["keyword_id"])) > 1 for r in want[0])
        ties += int(np.count_nonzero(want[0]["end_pos"][1:] == want[0]["end_pos"][:-1]))
        cut_texts += offsets.size > 2
        by_class += sum(any(not tc.is_literal(c) and c is not ANY for c in tpls[int(w)]) for w in want[0]["keyword_id"])
    print("matches %d, with failing cells %d, seeded more than once %d, ties in end_pos %d, trials with cuts %d, matches of templates with classes %d"
          % (matches, inexact, many_seeds, ties, cut_texts, by_class))
    assert matches > 500 and inexact > 200 and many_seeds > 50 and ties > 20 and cut_texts > 50 and by_class > 200


def test_a_match_seeded_by_two_pieces_comes_out_once_and_ties_are_ordered():
    # `ab` and `cd` both seed ab[0-9]cd; three templates end at one position: length descending, id ascending
    tpls = [[99, 100], [97, 98, DIGIT, 99, 100], [DIGIT, 99, 100], [ANY, 99, 100]]
    ks = [0, 1, 0, 0]
    kws, terms = tc.compile_templates(tpls, ks)
    assert terms[1] == [(1, 0, 2), (0, 3, 2)]
    text = b"ab7cd abXcd xx7cd"
    rec = tc.oracle_records([bytes(kw) for kw in kws], text)
    want = tc.templates(rec, text, tpls, ks, terms)
    same(want, tc.window_scan(text, tpls, ks))
    assert tc.seeds_of(rec, terms, 0, 1) == 2 and tc.seeds_of(rec, terms, 6, 1) == 2
    assert [tuple(r) for r in want[0][:4].tolist()] == [(4, 5, 1), (4, 3, 2), (4, 3, 3), (4, 2, 0)] and want[1][:4].tolist() == [0, 0, 0, 0]
    assert (10, 5, 1) in [tuple(r) for r in want[0].tolist()] and want[1][[tuple(r) for r in want[0].tolist()].index((10, 5, 1))] == 1
    same(binding.templates_records(rec, TemplateSet(tpls, ks, terms), text, n_keywords=len(kws)), want)
    # an incomplete term set loses matches by the seed condition: that is defined
    first = [terms[0], terms[1][:1], terms[2], terms[3]]
    text2 = b"ab7cd Xb7cd abXcX"
    rec2 = tc.oracle_records([bytes(kw) for kw in kws], text2)
    want2 = tc.templates(rec2, text2, tpls, ks, first)
    assert want2[0].size < tc.window_scan(text2, tpls, ks)[0].size
    same(binding.templates_records(rec2, TemplateSet(tpls, ks, first), text2, n_keywords=len(kws)), want2)


def test_counting_only_overflow_and_dist_null(novel_bytes):
    text = novel_bytes[:6000]
    tpls, ks = [template(r"[A-Z][a-z]{2}\.\sDalloway"), template(r"th[aeiou]\s"), [ord("C"), ANY, ord("a"), SymbolClass([(97, 122)], negate=True)]], [1, 0, 1]
    kws, terms = tc.compile_templates(tpls, ks)
    rec = tc.oracle_records([bytes(kw) for kw in kws], text)
    want = tc.templates(rec, text, tpls, ks, terms)
    same(want, tc.window_scan(text, tpls, ks), "the two derivations")
    per = np.bincount(want[0]["keyword_id"], minlength=3)
    print("records %d, matches per template %s, with failing cells %d" % (rec.size, per.tolist(), int(np.count_nonzero(want[1]))))
    assert np.all(per > 0) and np.count_nonzero(want[1]) > 0
    tset = TemplateSet(tpls, ks, terms)
    same(binding.templates_records(rec, tset, text, n_keywords=len(kws)), want)
    L = acm.lib()
    t = np.frombuffer(text, np.uint8)
    n = C.c_uint64(0)
    total = want[0].size

    def call(out, dist, cap, records=rec, n_symbols=len(text), pos_base=0, off=None, n_texts=0, sym_bytes=1):
        return L.acm_templates_records(records.ctypes.data, records.size, t.ctypes.data, sym_bytes, n_symbols, pos_base,
                                       off.ctypes.data if off is not None else None, n_texts, *tset.args(), len(kws),
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
    shifted, moved = rec.copy(), want[0].copy()                                  # a nonzero pos_base
    shifted["end_pos"] += 1 << 40
    moved["end_pos"] += 1 << 40
    same(binding.templates_records(shifted, tset, text, pos_base=1 << 40, n_keywords=len(kws)), (moved, want[1]))
    # acm_approx_records' argument errors: records outside the buffer or of length 0, offsets that break the contract
    assert call(out, dist, total, records=shifted) == E_ARG
    zero = rec.copy()
    zero["length"][3] = 0
    assert call(out, dist, total, records=zero) == E_ARG
    assert call(out, dist, total, sym_bytes=0) == E_ARG
    for off in ([0, 10, 5, len(text)], [1, len(text)], [0, len(text) - 1]):
        assert call(out, dist, total, off=np.array(off, np.uint64), n_texts=len(off) - 1) == E_ARG
    same((out, dist), want)                                                      # nothing was written by the refused calls


def test_wider_symbols_compare_all_their_bytes():
    for sb, dt in ((2, np.uint16), (4, np.uint32), (8, np.uint64)):
        hi = 0x41 << (8 * sb - 8)
        top = (1 << (8 * sb)) - 1
        high_only = SymbolClass([(hi | 0x30, hi | 0x39)])                          # digits under the high byte: a low-byte compare accepts plain digits
        ends = SymbolClass([(0, 0), (top, top)])
        tpl = [hi | 97, hi | 98, high_only, ends, hi | 99]
        text = np.array([hi | 97, hi | 98, hi | 0x35, 0, hi | 99, hi | 97, hi | 98, 0x35, top, hi | 99, hi | 97, hi | 98, hi | 0x35, 1, hi | 99, 0], dtype=dt)
        kws, terms = tc.compile_templates([tpl], [1])
        rec = tc.brute(kws, text)
        want = tc.templates(rec, text, [tpl], [1], terms)
        same(want, tc.window_scan(text, [tpl], [1]))
        assert want[1].tolist() == [0, 1, 1]
        same(binding.templates_records(rec, TemplateSet([tpl], [1], terms, sym_size=sb), text, n_keywords=len(kws)), want, sb)


def test_from_templates_cuts_canonically_and_reuses_ids():
    m = acm.Machine(1)
    m.add_keyword(b"cd")
    tpls, ks = [template(r"ab\dcd"), template("abcd[xy]efgh"), template(".ab")], [1, 2, 0]
    tset = TemplateSet.from_templates(m, tpls, ks)
    kws, terms = tc.compile_templates(tpls, ks, keywords=[tuple(b"cd")])
    assert [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws and tset.n_keywords == len(kws)
    assert tset.terms.tolist() == [list(t) for p in terms for t in p] and tset.tgt_ptr.tolist() == [0, 2, 5, 6] and tset.k.tolist() == ks
    assert terms[0] == [(1, 0, 2), (0, 3, 2)]                                    # `cd` keeps its id
    tset.check(m.nb_keywords)
    m4 = acm.Machine(4)
    t4 = TemplateSet.from_templates(m4, [[70000, 70001, SymbolClass([(1 << 20, 1 << 21)]), 5]], 1)
    assert t4.sym_size == 4 and t4.terms.tolist() == [[0, 0, 1], [1, 1, 1]] and t4.spell_data.dtype == np.uint32 and t4.ranges.dtype == np.uint32


def test_template_parses_the_fixed_length_subset():
    W = SymbolClass([(48, 57), (65, 90), (95, 95), (97, 122)])
    S = SymbolClass([(9, 13), (32, 32)])
    assert template("ab") == [97, 98] and template(b"a.") == [97, ANY]
    assert template(r"\d{3}-\d{2}-\d{4}") == [DIGIT] * 3 + [45] + [DIGIT] * 2 + [45] + [DIGIT] * 4
    assert template(r"[a-z0-9_]x") == [SymbolClass([(97, 122), (48, 57), (95, 95)]), 120]
    assert template(r"[^ab]") == [SymbolClass([(97, 97), (98, 98)], negate=True)]
    assert template(r"\w\s\D") == [W, S, SymbolClass([(48, 57)], negate=True)]
    assert template(r"[\d\-x]") == [SymbolClass([(48, 57), (45, 45), (120, 120)])]
    assert template(r"[a-]") == [SymbolClass([(97, 97), (45, 45)])]
    assert template(r"\x41\xff[\x00-\x1f]") == [0x41, 0xFF, SymbolClass([(0, 31)])]
    assert template(r"\.\*\+\?\|\(\)\[\]\{\}\\\^\$") == [ord(c) for c in ".*+?|()[]{}\\^$"]
    assert template(r"a\n\t\0") == [97, 10, 9, 0]
    assert template("a{1}b{0}c{3}") == [97, 99, 99, 99] and template(r"20\d\d-[01]\d-[0-3]\d")[5] == SymbolClass([48, 49])
    assert template("") == []
    for bad in ("a*", "a+", "a?", "a|b", "(a)", "a{1,2}", "a{2,}", "a{,2}", "{2}", "a{x}", "a{2", "^a", "a$", "[a", "[]", "[^]", "a]", "a}", "[z-a]",
                "[a-\\d]", "[[a]]", r"\b", r"\A", r"\1", r"[\D]", "\\", r"\x4", r"\xg1", "Ā"):
        with pytest.raises(ValueError):
            template(bad)
    with pytest.raises(ValueError):
        template("[" + "".join("\\x%02x" % (2 * i) for i in range(17)) + "]")   # 17 ranges
    assert len(template("[" + "".join("\\x%02x" % (2 * i) for i in range(16)) + "]")[0].ranges) == 16


def test_hex_template_and_iupac():
    assert hex_template("E2 3? ?? [C0-CF] A1") == [0xE2, SymbolClass([(0x30, 0x3F)]), ANY, SymbolClass([(0xC0, 0xCF)]), 0xA1]
    low = hex_template("?3")[0]
    assert [x for x in range(256) if tc.accepts(low, x)] == list(range(3, 256, 16)) and len(low.ranges) == 16
    assert hex_template("") == [] and hex_template("  0a\tFf ") == [10, 255]
    for bad in ("E", "E2A1", "G1", "[C0-CF", "[CF-C0]", "[C-CF]", "???", "3?? "):
        with pytest.raises(ValueError):
            hex_template(bad)
    assert sorted(IUPAC) == sorted("ACGTRYSWKMBDHVN") and IUPAC["N"] is ANY and IUPAC["A"] == 65
    sets = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
    for code, members in sets.items():
        assert [chr(x) for x in range(256) if tc.accepts(IUPAC[code], x)] == sorted(members)
    # a primer with a mismatch budget, through the whole host pass
    primer, text = [IUPAC[c] for c in "GGNRYCCA"], b"GGAGTCCA GGTACCCA GGCCTCCA GGAGTCCT GGAGGCCT"
    kws, terms = tc.compile_templates([primer], [1])
    want = tc.templates(tc.oracle_records([bytes(kw) for kw in kws], text), text, [primer], [1], terms)
    same(want, tc.window_scan(text, [primer], [1]))
    assert want[0]["end_pos"].tolist() == [7, 16, 25, 34] and want[1].tolist() == [0, 0, 1, 1]
    m = acm.Machine(1)
    tset = TemplateSet.from_templates(m, [primer], 1)
    same(binding.templates_records(tc.oracle_records([bytes(kw) for kw in kws], text), tset, text), want)


@pytest.mark.parametrize("pattern,least", [(r"\d{3}-\d{2}-\d{4}", 3), (r"[A-Z][a-z]{3} Dalloway", 0), (r"[A-Z][a-z]{2}\.\sDalloway", 3),
                                           (r"th[^aeiou\s].\w", 3), (r"[\x00-\x20]M[a-z]{2}\.", 3), (r"\s\S\W\D", 3)])
def test_template_reads_a_pattern_as_re_does(novel_bytes, pattern, least):
    """(the fixture separates words by tabs, so the second pattern matches nowhere in it: both sides must say so)"""
    text = novel_bytes[:200000] + b" 078-05-1120, 219-09-9999 and 1234-56-78901 but not 12-345-6789; 000-00-00000"
    cells = template(pattern)
    want = tc.regex_scan(pattern.encode("latin-1"), text, len(cells))
    print("%s: %d matches" % (pattern, want[0].size))
    assert want[0].size >= least
    if any(tc.is_literal(c) for c in cells):
        kws, terms = tc.compile_templates([cells], [0])
        rec = tc.oracle_records([bytes(kw) for kw in kws], text)
        same(binding.templates_records(rec, TemplateSet([cells], 0, terms), text, n_keywords=len(kws)), want, pattern)
    else:                                                                        # no literal cell, no seed: the cells against re through the window scan
        same(tc.window_scan(text, [cells], [0]), want, pattern)


def _scan_templates(h, text, tset, cap, offsets=None):
    out, dist = np.zeros(max(cap, 1), po.RECORD_DTYPE), np.zeros(max(cap, 1), np.uint32)
    n = C.c_uint64(0)
    off = np.ascontiguousarray(offsets, np.uint64) if offsets is not None else None
    rc = acm.lib().acm_scan_templates(h, text.ctypes.data if text.size else None, text.size, off.ctypes.data if off is not None else None,
                                      off.size - 1 if off is not None else 0, *tset.args(), out.ctypes.data if cap else None, dist.ctypes.data, cap,
                                      C.byref(n))
    return rc, int(n.value), (out[:min(int(n.value), cap)], dist[:min(int(n.value), cap)])


def test_acm_scan_templates_on_a_case_insensitive_machine_folds_literals_but_not_classes(kat):
    m = acm.Machine(1, cmp=C.cast(kat.kat_casecmp8, C.c_void_p))
    upper = SymbolClass([(65, 90)])
    tpls, ks = [[ord(c) for c in "mrs"] + [ANY, upper] + [ord(c) for c in "allo"], [ord(c) for c in "id-"] + [DIGIT] * 2], [1, 0]
    tset = TemplateSet.from_templates(m, tpls, ks)
    text = b"Mrs Dalloway MRS.DALLOWAY mrs dalloway mrs Xallo mrx Qallo ID-42 id-4x Id-07"
    t = np.frombuffer(text, np.uint8)
    assert acm.lib().acm_scan_templates(m.handle, t.ctypes.data, t.size, None, 0, *tset.args(), None, None, 0, C.byref(C.c_uint64(0))) == E_INELIGIBLE
    m.set_symbol_bytes(1)
    # literals fold: the expected answer reads a lower-cased text with the literal cells, and the caller's text with the class cells
    low = text.lower()
    want = []
    for w, cells in enumerate(tpls):
        for S in range(len(text) - len(cells) + 1):
            d = sum(not tc.accepts(c, (low if tc.is_literal(c) else text)[S + i]) for i, c in enumerate(cells))
            if d <= ks[w]:
                want.append((S + len(cells) - 1, len(cells), w, d))
    want = tc.ordered(want)
    assert [tuple(r) for r in want[0].tolist()] == [(8, 9, 0), (21, 9, 0), (34, 9, 0), (47, 9, 0), (57, 9, 0), (63, 5, 1), (75, 5, 1)]
    assert want[1].tolist() == [0, 0, 1, 0, 1, 0, 0]                             # `mrs dalloway`: the class cell does not fold, one failing cell
    rc, n, got = _scan_templates(m.handle, t, tset, want[0].size)
    assert rc == 0 and m.scan_path == PATH_LOOP
    same(got, want)
    same(m.scan_templates(text, tset), want)
    rc, n, got = _scan_templates(m.handle, t, tset, want[0].size - 1)
    assert rc == E_OVERFLOW and n == want[0].size
    assert _scan_templates(m.handle, t, tset, 0)[:2] == (0, want[0].size)
    offsets = np.array([0, 0, 5, 21, len(text)], np.uint64)                      # a batch: a cut inside the first match
    cut = _scan_templates(m.handle, t, tset, want[0].size, offsets=offsets)[2]
    assert [tuple(r) for r in cut[0].tolist()] == [tuple(r) for r in want[0].tolist()][2:]
    # this call knows the machine: a term whose keyword is not spelled as its piece is an argument error
    moved = TemplateSet(tpls, ks, [[(0, 1, 1), (1, 5, 2)], [(2, 0, 3)]])
    assert _scan_templates(m.handle, t, moved, 8)[0] == E_ARG
    assert _scan_templates(m.handle, t, tset, 8, offsets=[0, 7, 5, len(text)])[0] == E_ARG
