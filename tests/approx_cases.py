"""Shared by the approximate-match tests (test_approx_cpu.py, test_approx_gpu.py): the expected answer, which is
always the DEFINITION of APPROX (include/acm_gpu.h) in plain Python over the oracle's / tests/brute.py's record
set -- never the library's own scan or join --, a second, independent derivation from the text alone (a
brute-force Hamming scan per text, valid for canonical cuts, where the seed condition follows from the other
two), and the canonical cut done here in plain Python, so that the binding's own ApproxSet.from_targets is
checked against it and not against itself."""
import numpy as np

from oracle import pyoracle as po
from tests.brute import brute_records


def split(L, k):
    """the canonical cut of L symbols into k + 1 pieces: [(begin, end)]"""
    assert L >= k + 1
    return [(j * L // (k + 1), (j + 1) * L // (k + 1)) for j in range(k + 1)]


def compile_targets(targets, ks, keywords=()):
    """(keywords, terms): the distinct pieces of all targets in order of first appearance behind the given
    `keywords` (tuples of symbol values), and per target its terms (keyword_id, offset, length)"""
    kws = [tuple(int(x) for x in kw) for kw in keywords]
    terms = []
    for tgt, k in zip(targets, ks):
        sym = tuple(int(x) for x in tgt)
        mine = []
        for b, e in split(len(sym), k):
            if sym[b:e] not in kws:
                kws.append(sym[b:e])
            mine.append((kws.index(sym[b:e]), b, e - b))
        terms.append(mine)
    return kws, terms


def ordered(quads):
    """(records, dist) of (end_pos, length, target, d) in the total order"""
    quads = sorted(quads, key=lambda r: (r[0], -r[1], r[2]))
    rec = np.array([q[:3] for q in quads], dtype=po.RECORD_DTYPE) if quads else np.zeros(0, po.RECORD_DTYPE)
    return rec, np.array([q[3] for q in quads], dtype=np.uint32)


def approx(records, text, targets, ks, terms, offsets=None, pos_base=0):
    """APPROX by its definition: target w matches at S iff some text holds [S, S + L_w), some term's record is in
    the record set and at most k[w] symbols differ; (records, dist) in the total order"""
    R = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)}
    text = [int(x) for x in text]
    n = len(text)
    off = [0, n] if offsets is None else [int(x) for x in offsets]
    out = []
    for w, tgt in enumerate(targets):
        sym = [int(x) for x in tgt]
        L = len(sym)
        for S in range(0, n - L + 1):
            if not any(off[t] <= S and S + L <= off[t + 1] for t in range(len(off) - 1)):
                continue
            if not any((pos_base + S + o + l - 1, l, kid) in R for kid, o, l in terms[w]):
                continue
            d = sum(1 for i in range(L) if text[S + i] != sym[i])
            if d <= ks[w]:
                out.append((pos_base + S + L - 1, L, w, d))
    return ordered(out)


def seeds_of(records, targets, terms, S, w, pos_base=0):
    """how many terms of target w seed a match at S"""
    R = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)}
    return sum((pos_base + S + o + l - 1, l, kid) in R for kid, o, l in terms[w])


def hamming_scan(text, targets, ks, offsets=None, pos_base=0):
    """the same from the text alone, for canonical cuts: per text and target every window within the budget"""
    a = np.asarray([int(x) for x in text], dtype=np.uint64)
    off = [0, a.size] if offsets is None else [int(x) for x in offsets]
    out = []
    for w, tgt in enumerate(targets):
        sym = np.asarray([int(x) for x in tgt], dtype=np.uint64)
        L = sym.size
        for t in range(len(off) - 1):
            part = a[off[t]:off[t + 1]]
            if part.size < L:
                continue
            win = np.lib.stride_tricks.sliding_window_view(part, L)
            d = np.count_nonzero(win != sym, axis=1)
            for S in np.nonzero(d <= ks[w])[0]:
                out.append((pos_base + off[t] + int(S) + L - 1, L, w, int(d[S])))
    return ordered(out)


def same(got, want, what=None):
    """(records, dist) pairs are equal, order included"""
    (g, gd), (w, wd) = got, want
    assert g.size == w.size and np.array_equal(np.asarray(g).astype(po.RECORD_DTYPE), w), (what, g.size, w.size, g[:8], w[:8])
    assert np.array_equal(np.asarray(gd).astype(np.uint32), wd), (what, gd[:16], wd[:16])


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
    """(targets, ks, text, offsets) of the random check: 1 to 4 targets of 2 to 9 symbols over {a, b} with k of 0
    to 2 (below the target's length), a text of 0 to 60 symbols over {a, b} cut into 1 to 4 texts"""
    ab = np.frombuffer(b"ab", np.uint8)
    targets, ks = [], []
    for _ in range(int(rng.integers(1, 5))):
        L = int(rng.integers(2, 10))
        targets.append(bytes(rng.choice(ab, size=L)))
        ks.append(int(rng.integers(0, min(3, L))))
    n = int(rng.integers(0, 61))
    text = bytes(rng.choice(ab, size=n))
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 4))))
    offsets = np.array([0] + [int(c) for c in cuts] + [n], np.uint64)
    return targets, ks, text, offsets
