"""Shared by the position tests (test_positions_cpu.py, test_positions_gpu.py): texts placed so that
their record positions cross a 32-bit carry, with and without bit 63 set.

Every definition in include/acm_gpu.h states positions relative to pos_base (end_pos of a match ending
at buffer index i = pos_base + i), so the answer at a base B is the answer at base 0 translated by B.
The expected answer here is therefore always the family's own Python definition (tests/*_cases.py)
over the ORACLE's records at pos_base = 0, then moved() -- never the library's output at another base,
and never the Python definitions evaluated at the high base (they compute in int64)."""
import numpy as np

U64 = (1 << 64) - 1
NAMES = ("WRAP32", "TOP")


def bases(c, len_bits=None):
    """the named bases that put buffer index c on a boundary: WRAP32 -- index c is position 2^32, the low
    word of every position from there on has wrapped; TOP -- the same with bit 63 set; SORT_EDGE (with
    len_bits, the sort tests only) -- index c is position 2^(64 - len_bits), the first that a key of
    (position << len_bits | ...) cannot hold"""
    c = int(c)
    b = {"WRAP32": (1 << 32) - c, "TOP": (1 << 63) + (1 << 32) - c}
    if len_bits is not None:
        b["SORT_EDGE"] = (1 << (64 - int(len_bits))) - c
    assert all(0 < v and v + c <= U64 for v in b.values()), (c, b)
    return b


def moved(x, base, fields=("end_pos",)):
    """a copy of x translated by base in np.uint64: the fields `fields` of a structured array (end_pos,
    tok_start, ...), or every element of a plain array of positions"""
    x = np.asarray(x)
    base = np.uint64(int(base) & U64)
    if x.dtype.names is None:
        return (x.astype(np.uint64) + base).astype(np.uint64)
    out = x.copy()
    for f in fields:
        out[f] = (out[f].astype(np.uint64) + base).astype(out.dtype[f])
    return out


def _three(start, end, c, what):
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    below, above, across = int(np.count_nonzero(end < c)), int(np.count_nonzero(end >= c)), int(np.count_nonzero((start < c) & (c <= end)))
    print("%s: %d end below index %d, %d at or above it, %d lie across it" % (what, below, c, above, across))
    assert below >= 1, "%s: nothing ends below index %d" % (what, c)
    assert above >= 1, "%s: nothing ends at or above index %d" % (what, c)
    assert across >= 1, "%s: nothing has start < %d <= end" % (what, c)


def straddles(rec, c, out=None):
    """From the oracle alone (records at pos_base = 0): the boundary at buffer index c has records ending
    on both sides of it and one lying across it.  out: (first index, last index) arrays of the EXPECTED
    output's extents (selected records, matches, chains, snippets, tokens, replaced spans), held to the
    same three conditions.  Conditions, not measurements: a case that fails them gets another c."""
    rec = np.asarray(rec)
    end = rec["end_pos"].astype(np.int64)
    _three(end + 1 - rec["length"].astype(np.int64), end, int(c), "records")
    if out is not None:
        _three(out[0], out[1], int(c), "expected output")


def extent(rec):
    """(first index, last index) of records, for straddles(out=)"""
    end = np.asarray(rec["end_pos"]).astype(np.int64)
    return end + 1 - np.asarray(rec["length"]).astype(np.int64), end


def boundary_inside(rec, near, min_length=2):
    """a buffer index c with start < c <= end for the record of at least min_length symbols whose end is
    closest to `near`: c = that record's end"""
    rec = np.asarray(rec)
    ok = np.flatnonzero(rec["length"] >= min_length)
    assert ok.size, "no record of %d symbols or more" % min_length
    end = rec["end_pos"][ok].astype(np.int64)
    return int(end[np.argmin(np.abs(end - int(near)))])


def canonical(rec):
    """np.sort by (end_pos ascending, length descending, keyword_id) on the host, in full 64 bits"""
    rec = np.asarray(rec)
    key = np.zeros(rec.size, dtype=[("end_pos", np.uint64), ("neg_length", np.int64), ("keyword_id", np.uint32)])
    key["end_pos"], key["neg_length"], key["keyword_id"] = rec["end_pos"], -rec["length"].astype(np.int64), rec["keyword_id"]
    return rec[np.argsort(key, order=("end_pos", "neg_length", "keyword_id"), kind="stable")]


def breach_positions(base, n_symbols, in_range_index):
    """positions that break the contract pos_base <= pos < pos_base + n_symbols at a high base: the two
    whose LOW word is that of a valid position and whose high word is wrong, and the two just outside"""
    base, p = int(base), int(base) + int(in_range_index)
    return [(p - (1 << 32)) & U64, (p + (1 << 32)) & U64, (base - 1) & U64, (base + int(n_symbols)) & U64]


# ---------------------------------------------------------------- the families' cases
# Small texts with planted occurrences, as bytes and as 4-byte symbols with a high byte set in every
# symbol (a compare of the low byte alone is seen).  Every case is made once; arrays are left unchanged.
HIGH = {1: 0, 4: 0x41000000}
SYM = {1: np.uint8, 4: np.uint32}
WORD_KEYWORDS = [b"he", b"she", b"his", b"hers", b"the", b"e.g.", b"New York", b"x"]
WORD_TEXT = b"the she he, her hers_he e.g. New York's New York x xx ax x_ _x (x) ushers e.g.x his " * 7
WORD_RANGES = ((0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A))
SEGMENT_COST, SEGMENT_GAP = [3, 2, 4, 1, 5, 9, 2, 6], 2
REPLACEMENTS = [b"HE", b"SHE", b"HIS", b"HERS", b"THE", b"eg", b"NY", b""]
TOKEN_GAP_BASE = 1000
PATTERN_TEMPLATES = [b"a?c", b"ab?d", b"a?cd", b"b?d", b"a??d", b"?bc"]
PATTERN_TEXT = b"abcd abxd axcd xbc ab aabcdd bcd b?d abbd acc abc " * 6
APPROX_TARGETS, APPROX_KS = [b"abcdefgh", b"defgh ab", b"Xbcd"], [1, 2, 1]
APPROX_TEXT = b"abcdefgh abcdeXgh abXdefgh Xbcdefgh abcdXfgh abXdeXgh abcdfgh abcdeefgh " * 5


def sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(SYM[sb])


def ranges_of(sb):
    return [(lo | HIGH[sb], hi | HIGH[sb]) for lo, hi in WORD_RANGES]


def oracle_of(keywords, sb):
    from oracle import pyoracle as po
    o = po.Oracle(sb, po.AC75)
    for kw in keywords:
        o.add_keyword(np.asarray(kw, SYM[sb]) if not isinstance(kw, (bytes, bytearray)) else kw)
    return o


def frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def thirds(n, c=None):
    """offsets that cut a buffer of n symbols into three texts and two empty ones; with c, the middle
    cut is moved onto c: the carry falls exactly on a text boundary"""
    a, b = (n // 3, 2 * n // 3) if c is None else (n // 4, int(c))
    assert 0 < a < b < n
    return np.array([0, a, a, b, b, n], np.uint64)


def _cached(fn):
    import functools
    return functools.lru_cache(maxsize=None)(fn)


@_cached
def word_case(sb):
    """(keywords, text, the oracle, its records of the text) of the families that take a record set and
    the text: select, segment, words, context, replace, tokens"""
    kws = [sym(k, sb) for k in WORD_KEYWORDS]
    text = frozen(sym(WORD_TEXT, sb))
    o = oracle_of(kws, sb)
    return kws, text, o, frozen(o.scan(text))


def replacements_of(sb):
    return [sym(r, sb) for r in REPLACEMENTS]


@_cached
def pattern_case():
    from tests.pattern_cases import compile_templates
    kws, pats = compile_templates(PATTERN_TEMPLATES)
    text = frozen(np.frombuffer(PATTERN_TEXT, np.uint8))
    return kws, pats, text, frozen(oracle_of([bytes(k) for k in kws], 1).scan(text))


@_cached
def chain_case():
    from tests.chain_cases import CASE_CHAINS, CASE_KEYWORDS, CASE_TEXT
    text = frozen(np.frombuffer(CASE_TEXT * 3, np.uint8))
    return CASE_KEYWORDS, CASE_CHAINS, text, frozen(oracle_of(CASE_KEYWORDS, 1).scan(text))


@_cached
def approx_case(sb):
    """(targets, budgets, (keywords, terms) of the canonical cut, text, the oracle's records): approx and edit"""
    from tests.approx_cases import compile_targets
    targets = [sym(t, sb) for t in APPROX_TARGETS]
    kws, terms = compile_targets(targets, APPROX_KS)
    text = frozen(sym(APPROX_TEXT, sb))
    return targets, list(APPROX_KS), (kws, terms), text, frozen(oracle_of([np.array(k, SYM[sb]) for k in kws], sb).scan(text))


@_cached
def template_case(sb):
    from aho_corasick_1975_amd.binding import ANY, SymbolClass
    from tests.template_cases import compile_templates
    hi = HIGH[sb]
    a, b, c, d, e, f, g, h, X = (x | hi for x in b"abcdefghX")
    tpls = [[a, b, ANY, d, e, SymbolClass([(f, g)]), g, h], [SymbolClass([a, X]), b, c, d], [d, e, SymbolClass([f], negate=True), g, h]]
    ks = [1, 0, 1]
    kws, terms = compile_templates(tpls, ks)
    text = frozen(sym(APPROX_TEXT, sb))
    return tpls, ks, (kws, terms), text, frozen(oracle_of([np.array(k, SYM[sb]) for k in kws], sb).scan(text))


# ---------------------------------------------------------------- the core scan's cases
N_SCAN = 1 << 16


def scan_case(name, monkeypatch, kat, novel_bytes, device=None):
    """A plan kind of tests/tally_cases.KINDS on the first 64 Ki symbols of its text -- eight 8,192-symbol
    tiles, sixteen 4,096-position buckets: the smallest shape that still has seams -- with the boundary c
    inside a planted keyword near the middle.  Returns (machine, oracle, text, c, the oracle's records) and,
    with `device`, the plan behind them (made BEFORE the oracle scans: the delta kind adds keywords then)."""
    from tests.tally_cases import kind
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    text = frozen(np.ascontiguousarray(text[1:N_SCAN + 1] if name == "csr" else text[:N_SCAN]))
    plan = None
    if device is not None:
        plan = make_plan(device)
        assert plan_ok(plan), plan.describe()
    rec = frozen(o.scan(text))
    c = boundary_inside(rec, N_SCAN // 2)
    straddles(rec, c)
    assert abs(c - N_SCAN // 2) < 4096 and c > 3
    return (m, o, text, c, rec) + ((plan,) if device is not None else ())


# ---------------------------------------------------------------- the families' expected answers
def _binding():
    from aho_corasick_1975_amd import binding
    return binding


def _record_dtype():
    from oracle import pyoracle as po
    return po.RECORD_DTYPE


FAMILIES = ["select", "segment", "words", "context", "replace", "tokens", "patterns", "chains", "approx", "edit", "templates"]
TEXT_FAMILIES = ["words", "context", "replace", "tokens", "approx", "edit", "templates"]      # they index the text by pos - pos_base
BATCH_FAMILIES = ["words", "context", "tokens", "patterns", "chains", "approx", "edit", "templates"]   # their record calls take offsets
CONTEXT_BEFORE, CONTEXT_AFTER = 0, 1


class Want:
    """the expected answer of a family at pos_base = 0: `records` (what moves with the base, or None), `rest`
    (arrays that do not depend on the base), `starts` (tok_start: moves with the base, or None), `extent` of
    the output for straddles(), and the input records `rec` (for replace and tokens the selection)"""

    def __init__(self, rec, records=None, rest=(), starts=None, out_extent=None):
        self.rec, self.records, self.rest, self.starts = rec, records, tuple(rest), starts
        self.extent = out_extent if out_extent is not None else extent(records)

    def at(self, base):
        return (None if self.records is None else moved(self.records, base), self.rest, None if self.starts is None else moved(self.starts, base))


def inputs(family, sb):
    """(text, all the oracle's records of it) of a family's case"""
    if family == "patterns":
        return pattern_case()[2:]
    if family == "chains":
        return chain_case()[2:]
    if family in ("approx", "edit"):
        return approx_case(sb)[3:]
    if family == "templates":
        return template_case(sb)[3:]
    return word_case(sb)[1::2]


def want_of(family, sb, offsets=None):
    """the family's definition (tests/*_cases.py) over the oracle's records at pos_base = 0"""
    from tests.approx_cases import approx
    from tests.chain_cases import chains
    from tests.context_cases import expected
    from tests.edit_cases import edits
    from tests.pattern_cases import patterns
    from tests.replace_cases import replace_by_definition
    from tests.segment_cases import define
    from tests.select_cases import greedy
    from tests.template_cases import templates
    from tests.token_cases import RUN, selection_of, tokens_by_definition
    from tests.words_cases import words
    text, rec = inputs(family, sb)
    n = text.size
    if family == "select":
        return Want(rec, greedy(rec))
    if family == "segment":
        out, cost = define(rec, SEGMENT_COST, SEGMENT_GAP, 0, n)
        return Want(rec, out, [np.array([cost - SEGMENT_GAP * (n - int(out["length"].sum())), int(out["length"].sum())], np.uint64)])
    if family == "words":
        return Want(rec, words(rec, text, offsets, ranges_of(sb)))
    if family == "context":
        exp = expected(rec, n, offsets, CONTEXT_BEFORE, CONTEXT_AFTER)
        lo, lens = exp.snip_lo.astype(np.int64), exp.lens.astype(np.int64)
        return Want(rec, None, [exp.snip_lo, exp.out_offsets, exp.snip_text, exp.rec_snip, exp.rec_at, exp.out(text)], out_extent=(lo, lo + lens - 1))
    if family in ("replace", "tokens"):
        o = word_case(sb)[2]
        all_rec, sel = selection_of(o, text, offsets)
        if family == "replace":
            out, starts = replace_by_definition(text, sel, replacements_of(sb))
            return Want(sel, None, [out, starts.astype(np.uint64)], out_extent=extent(sel))
        ids, starts, lens, first = tokens_by_definition(text, sel, RUN, TOKEN_GAP_BASE, None, offsets)
        s = starts.astype(np.int64)
        return Want(sel, None, [ids, lens] + ([first] if first is not None else []), starts=starts, out_extent=(s, s + lens.astype(np.int64) - 1))
    if family == "patterns":
        return Want(rec, patterns(rec, pattern_case()[1], n, offsets))
    if family == "chains":
        return Want(rec, chains(rec, chain_case()[1], n, offsets))
    if family in ("approx", "edit"):
        targets, ks, (kws, terms), _, _ = approx_case(sb)
        out, dist = (approx if family == "approx" else edits)(rec, text, targets, ks, terms, offsets)
        return Want(rec, out, [dist])
    assert family == "templates"
    tpls, ks, (kws, terms), _, _ = template_case(sb)
    out, dist = templates(rec, text, tpls, ks, terms, offsets)
    return Want(rec, out, [dist])


def boundary_of(family, sb):
    """the buffer index the carry is put on: inside an occurrence near the middle of the text -- inside a
    record of the expected output where the output is records, so that both straddle"""
    w = want_of(family, sb)
    n = inputs(family, sb)[0].size
    c = boundary_inside(w.records if w.records is not None else w.rec, n // 2)
    straddles(inputs(family, sb)[1], c, w.extent)
    return c


def sets_of(family, sb):
    """the compiled set a family's calls take (None for the families without one), and the number of keywords"""
    if family == "patterns":
        kws, pats = pattern_case()[:2]
        return _binding().PatternSet(pats), len(kws)
    if family == "chains":
        kws, chain_list = chain_case()[:2]
        return _binding().ChainSet(chain_list), len(kws)
    if family in ("approx", "edit"):
        targets, ks, (kws, terms) = approx_case(sb)[:3]
        return _binding().ApproxSet(targets, ks, terms), len(kws)
    if family == "templates":
        tpls, ks, (kws, terms) = template_case(sb)[:3]
        return _binding().TemplateSet(tpls, ks, terms, sym_size=sb), len(kws)
    return None, len(WORD_KEYWORDS)


def same(got, want, what):
    """(records, rest, starts) triples are equal, element for element.  An entry of `rest` that the call does
    not return at all is given as None (acm_replace_records has no out_start)"""
    (g_rec, g_rest, g_start), (w_rec, w_rest, w_start) = got, want
    assert (g_rec is None) == (w_rec is None) and (g_start is None) == (w_start is None), what
    if w_rec is not None:
        g = np.asarray(g_rec).astype(_record_dtype())
        assert g.size == w_rec.size and np.array_equal(g, w_rec), (what, g.size, w_rec.size, g[:6], w_rec[:6])
    assert len(g_rest) == len(w_rest), (what, len(g_rest), len(w_rest))
    for i, (g, w) in enumerate(zip(g_rest, w_rest)):
        if g is None:
            continue
        assert np.array_equal(np.asarray(g).astype(np.asarray(w).dtype), w), (what, "array %d" % i, np.asarray(g)[:8], np.asarray(w)[:8])
    if w_start is not None:
        assert np.array_equal(np.asarray(g_start).astype(np.uint64), w_start), (what, np.asarray(g_start)[:8], w_start[:8])
