"""Shared by the template tests (test_templates_cpu.py, test_templates_gpu.py).  Expected answers never come from
the library: (a) TEMPLATES by its definition (include/acm_gpu.h) in plain Python over the oracle's / tests/brute.py's
record set; (b) a window scan from the text alone -- a numpy acceptance matrix per template --, valid for canonical
cuts, where the seed condition follows from the other two; (c) the canonical cut in plain Python, so that
acm_templates_split and TemplateSet.from_templates are checked against it and not against themselves; (d) for byte
templates with k = 0, Python's `re` with a lookahead, so that overlapping matches count: an implementation that
is not ours, against which template()'s parser is checked.  A template here is a list of cells: an int (literal),
ANY, or a SymbolClass -- the binding's two classes serve as plain containers; what a cell accepts is decided here."""
import re

import numpy as np

from aho_corasick_1975_amd.binding import ANY, SymbolClass
from tests.approx_cases import brute, oracle_records, ordered, same  # noqa: F401  (re-exported to the tests)


def is_literal(cell):
    return cell is not ANY and not isinstance(cell, SymbolClass)


def accepts(cell, x):
    """whether a cell accepts symbol x"""
    if cell is ANY:
        return True
    if isinstance(cell, SymbolClass):
        return any(lo <= x <= hi for lo, hi in cell.ranges) != cell.negate
    return int(cell) == x


def literal_runs(cells):
    """[(begin, length)] of the maximal stretches of literal cells"""
    runs, i = [], 0
    while i < len(cells):
        if not is_literal(cells[i]):
            i += 1
            continue
        j = i
        while j < len(cells) and is_literal(cells[j]):
            j += 1
        runs.append((i, j - i))
        i = j
    return runs


def split(cells, k):
    """(c) the canonical cut: [(offset, length)] of the k + 1 pieces, or None with fewer than k + 1 literal cells"""
    runs = literal_runs(cells)
    if sum(n for _, n in runs) < k + 1:
        return None
    q = max(q for q in range(1, len(cells) + 1) if sum(n // q for _, n in runs) >= k + 1)
    pieces = [(b + i * q, q) for b, n in runs for i in range(n // q)]
    return pieces[:k + 1]


def compile_templates(templates, ks, keywords=()):
    """(keywords, terms): the distinct pieces of the canonical cuts in order of first appearance behind the given
    `keywords` (tuples of symbol values), and per template its terms (keyword_id, offset, length)"""
    kws = [tuple(int(x) for x in kw) for kw in keywords]
    terms = []
    for cells, k in zip(templates, ks):
        mine = []
        for o, n in split(cells, k):
            piece = tuple(int(c) for c in cells[o:o + n])
            if piece not in kws:
                kws.append(piece)
            mine.append((kws.index(piece), o, n))
        terms.append(mine)
    return kws, terms


def templates(records, text, tpls, ks, terms, offsets=None, pos_base=0):
    """(a) TEMPLATES by its definition: template w matches at S iff some text holds [S, S + L_w), some term's record
    is in the record set and at most k[w] cells do not accept their symbol; (records, dist) in the total order"""
    R = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)}
    text = [int(x) for x in text]
    n = len(text)
    off = [0, n] if offsets is None else [int(x) for x in offsets]
    out = []
    for w, cells in enumerate(tpls):
        L = len(cells)
        for S in range(0, n - L + 1):
            if not any(off[t] <= S and S + L <= off[t + 1] for t in range(len(off) - 1)):
                continue
            if not any((pos_base + S + o + l - 1, l, kid) in R for kid, o, l in terms[w]):
                continue
            d = sum(1 for i in range(L) if not accepts(cells[i], text[S + i]))
            if d <= ks[w]:
                out.append((pos_base + S + L - 1, L, w, d))
    return ordered(out)


def seeds_of(records, terms, S, w, pos_base=0):
    """how many terms of template w seed a match at S"""
    R = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)}
    return sum((pos_base + S + o + l - 1, l, kid) in R for kid, o, l in terms[w])


def window_scan(text, tpls, ks, offsets=None, pos_base=0):
    """(b) the same from the text alone, for canonical cuts: per template an acceptance matrix (cell x position) from
    numpy comparisons, and per text every window whose failing cells are within the budget"""
    a = np.asarray([int(x) for x in text], dtype=np.uint64)
    off = [0, a.size] if offsets is None else [int(x) for x in offsets]
    out = []
    for w, cells in enumerate(tpls):
        L = len(cells)
        acc = np.ones((L, a.size), dtype=bool)
        for i, c in enumerate(cells):
            if isinstance(c, SymbolClass):
                inside = np.zeros(a.size, dtype=bool)
                for lo, hi in c.ranges:
                    inside |= (a >= np.uint64(lo)) & (a <= np.uint64(hi))
                acc[i] = ~inside if c.negate else inside
            elif c is not ANY:
                acc[i] = a == np.uint64(int(c))
        for t in range(len(off) - 1):
            lo, hi = off[t], off[t + 1]
            if hi - lo < L:
                continue
            d = np.zeros(hi - lo - L + 1, dtype=np.int64)
            for i in range(L):
                d += ~acc[i, lo + i:hi - L + 1 + i]
            for S in np.nonzero(d <= ks[w])[0]:
                out.append((pos_base + lo + int(S) + L - 1, L, w, int(d[S])))
    return ordered(out)


def regex_scan(pattern, text, length):
    """(d) every place where the regular expression `pattern` (bytes, of fixed length `length`) matches, overlapping
    ones included, as (records, dist) of template 0 at distance 0"""
    out = []
    for m in re.finditer(b"(?=(" + pattern + b"))", bytes(text), re.DOTALL):
        assert len(m.group(1)) == length
        out.append((m.start() + length - 1, length, 0, 0))
    return ordered(out)


ABC_CLASSES = [SymbolClass([(97, 98)]), SymbolClass([(98, 99)]), SymbolClass([97, 99]), SymbolClass([98], negate=True),
               SymbolClass([(97, 99)], negate=True), SymbolClass([]), SymbolClass([], negate=True)]


def random_case(rng):
    """(templates, ks, text, offsets) of the random check: 1 to 4 templates of 2 to 9 cells over {a, b, c} with literal,
    any, class and negated-class cells and k of 0 to 2 (at least k + 1 cells are literal, so that the cut exists), a
    text of 0 to 60 symbols over {a, b, c} cut into 1 to 4 texts"""
    abc = np.frombuffer(b"abc", np.uint8)
    tpls, ks = [], []
    for _ in range(int(rng.integers(1, 5))):
        L = int(rng.integers(2, 10))
        cells = []
        for _ in range(L):
            kind = rng.random()
            if kind < 0.55:
                cells.append(int(rng.choice(abc)))
            elif kind < 0.65:
                cells.append(ANY)
            else:
                cells.append(ABC_CLASSES[int(rng.integers(0, len(ABC_CLASSES)))])
        if not any(is_literal(c) for c in cells):
            cells[int(rng.integers(0, L))] = int(rng.choice(abc))
        tpls.append(cells)
        ks.append(int(rng.integers(0, min(3, sum(is_literal(c) for c in cells)))))
    n = int(rng.integers(0, 61))
    text = bytes(rng.choice(abc, size=n))
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 4))))
    offsets = np.array([0] + [int(c) for c in cuts] + [n], np.uint64)
    return tpls, ks, text, offsets
