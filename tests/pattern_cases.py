"""Shared by the pattern tests (test_patterns_cpu.py, test_patterns_gpu.py): the expected answer, which is
always the DEFINITION of PATTERNS (include/acm_gpu.h) in plain Python over the oracle's / tests/brute.py's
record set -- never the library's own scan or join --, a second, independent derivation from the text alone
with Python's `re` for byte text, and the cutting of templates into fragments done here in plain Python, so
that the binding's own PatternSet.from_templates is checked against it and not against itself."""
import re

import numpy as np

from oracle import pyoracle as po
from tests.brute import brute_records

WILD = ord("?")


def runs_of(template, wildcard=WILD):
    """the maximal don't-care-free runs of a template: [(offset, symbols)]"""
    sym = [int(x) for x in template]
    runs, i = [], 0
    while i < len(sym):
        if sym[i] == wildcard:
            i += 1
            continue
        j = i
        while j < len(sym) and sym[j] != wildcard:
            j += 1
        runs.append((i, tuple(sym[i:j])))
        i = j
    return runs


def compile_templates(templates, wildcard=WILD, keywords=()):
    """(keywords, patterns): the distinct runs of all templates in order of first appearance behind the given
    `keywords` (tuples of symbol values), and per template its terms (keyword_id, offset, length)"""
    kws = [tuple(int(x) for x in k) for k in keywords]
    patterns = []
    for tpl in templates:
        terms = []
        for off, run in runs_of(tpl, wildcard):
            if run not in kws:
                kws.append(run)
            terms.append((kws.index(run), off, len(run)))
        assert terms and int(list(tpl)[-1]) != wildcard
        patterns.append(terms)
    return kws, patterns


def as_records(triples):
    return np.array(sorted(triples, key=lambda r: (r[0], -r[1], r[2])), dtype=po.RECORD_DTYPE) if triples else np.zeros(0, po.RECORD_DTYPE)


def patterns(records, pats, n_symbols, offsets=None, pos_base=0):
    """PATTERNS by its definition: for every pattern p and every buffer index S, p matches at S iff some text
    holds [S, S + L_p) and every term's record is in the record set; the output in the total order"""
    R = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)}
    off = [0, n_symbols] if offsets is None else [int(x) for x in offsets]
    out = []
    for p, terms in enumerate(pats):
        L = max(o + l for _, o, l in terms)
        for S in range(0, n_symbols - L + 1):
            if not any(off[t] <= S and S + L <= off[t + 1] for t in range(len(off) - 1)):
                continue
            if all((pos_base + S + o + l - 1, l, k) in R for k, o, l in terms):
                out.append((pos_base + S + L - 1, L, p))
    return as_records(out)


def patterns_by_re(templates, text, offsets=None, wildcard=b"?", pos_base=0):
    """the same for byte text from the text alone: per text and template every occurrence, overlapping ones
    included, of the template with each don't-care matching any one byte"""
    text = bytes(text)
    off = [0, len(text)] if offsets is None else [int(x) for x in offsets]
    out = []
    for p, tpl in enumerate(templates):
        tpl = bytes(tpl)
        rx = re.compile(b"(?=(" + b"".join(b"." if tpl[i:i + 1] == wildcard else re.escape(tpl[i:i + 1]) for i in range(len(tpl))) + b"))", re.S)
        for t in range(len(off) - 1):
            for m in rx.finditer(text[off[t]:off[t + 1]]):
                out.append((pos_base + off[t] + m.start() + len(tpl) - 1, len(tpl), p))
    return as_records(out)


def byte_oracle(keywords):
    o = po.Oracle(1, po.MEYER85)
    for kw in keywords:
        o.add_keyword(bytes(kw))
    return o


def oracle_records(keywords, text):
    """the oracle's records of a byte text (canonical order)"""
    return byte_oracle(keywords).scan(bytes(text)) if len(text) else np.zeros(0, po.RECORD_DTYPE)


def brute(keywords, text):
    """tests/brute.py's records of a text of any symbols (canonical order)"""
    return brute_records([list(k) for k in keywords], list(int(x) for x in text))


def random_case(rng):
    """(templates, text, offsets) of the random check: 1 to 4 templates of 1 to 7 symbols over {a, b, ?} that do
    not end in ?, a text of 0 to 60 symbols over {a, b} cut into 1 to 4 texts (empty texts included)"""
    templates = []
    for _ in range(int(rng.integers(1, 5))):
        n = int(rng.integers(1, 8))
        tpl = bytes(rng.choice(np.frombuffer(b"ab?", np.uint8), size=n))
        tpl = tpl[:-1] + bytes(rng.choice(np.frombuffer(b"ab", np.uint8), size=1))
        templates.append(tpl)
    n = int(rng.integers(0, 61))
    text = bytes(rng.choice(np.frombuffer(b"ab", np.uint8), size=n))
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 4))))
    offsets = np.array([0] + [int(c) for c in cuts] + [n], np.uint64)
    return templates, text, offsets
