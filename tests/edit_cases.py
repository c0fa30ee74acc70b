"""Shared by the edit-distance tests (test_edit_cpu.py, test_edit_gpu.py): the expected answer, which is always
the DEFINITION of EDIT (include/acm_gpu.h) in Python over the oracle's / tests/brute.py's record set -- a full
free-start Sellers pass per text and target with the largest-start rule, then the seed condition against the
record set; never the library's own scan or verification --, and a second, independent derivation from the text
alone: for every end and every start a plain two-row Levenshtein distance, valid for canonical cuts, where the
seed condition follows from the distance."""
import numpy as np

from tests.approx_cases import ordered

BIG = 1 << 32


def sellers(part, sym):
    """(D, s*) as arrays over the ends e of `part` (symbols): D = the least edit distance of `sym` to part[s .. e] over
    all s in [0, e + 1], s* = the largest s that attains it.  One row per target symbol; a cell is
    cost * BIG + (BIG - 1 - start), so one minimum takes the least cost and then the largest start."""
    n, L = len(part), len(sym)
    a = np.asarray(part, dtype=np.uint64)
    idx = np.arange(n + 1, dtype=np.int64)
    row = BIG - 1 - idx                                                   # row 0: cost 0, start c
    for i in range(1, L + 1):
        diag = np.empty(n + 1, dtype=np.int64)
        diag[0] = (n + L + 1) * BIG                                       # (no cell left of the text)
        diag[1:] = row[:-1] + np.where(a == np.uint64(sym[i - 1]), 0, BIG)
        v = np.minimum(diag, row + BIG)
        row = np.minimum.accumulate(v - idx * BIG) + idx * BIG            # the left neighbours, resolved
    return row[1:] // BIG, BIG - 1 - row[1:] % BIG


def edits(records, text, targets, ks, terms, offsets=None, pos_base=0, seeded=True):
    """EDIT by its definition: target w matches with end e iff D_w (e) <= k[w] in the text of e and some term's
    record seeds it; (records, dist) in the total order.  seeded=False leaves the seed condition out (what the
    definition comes to under canonical cuts over a full record set)."""
    R = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)} if seeded else None
    text = [int(x) for x in text]
    off = [0, len(text)] if offsets is None else [int(x) for x in offsets]
    out = []
    for w, tgt in enumerate(targets):
        sym = [int(x) for x in tgt]
        L, k = len(sym), ks[w]
        for t in range(len(off) - 1):
            lo, hi = off[t], off[t + 1]
            D, s = sellers(text[lo:hi], sym)
            for i in np.nonzero(D <= k)[0]:
                e = lo + int(i)
                if not seeded or seeds_of(R, (lo, hi), e, L, k, terms[w], pos_base):
                    out.append((pos_base + e, int(i) - int(s[i]) + 1, w, int(D[i])))
    return ordered(out)


def seeds_of(records, text_bounds, e, L, k, terms_w, pos_base=0):
    """how many (term, record) pairs seed the match of a target (L symbols, budget k, terms terms_w) with end e in
    the text [lo, hi)"""
    R = records if isinstance(records, set) else {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)}
    lo, hi = text_bounds
    n = 0
    for kid, o, l in terms_w:
        r = L - o - l
        for back in range(max(0, r - k), r + k + 1):
            q = e - back
            n += q - l + 1 >= lo and q < hi and (pos_base + q, l, kid) in R
    return n


def ed(a, b):
    """the unit-cost Levenshtein distance of two lists, two rows"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def edit_scan(text, targets, ks, offsets=None, pos_base=0):
    """the same from the text alone, for canonical cuts: per text, target and end the least ed () over every start
    of that text, and the largest start that attains it.  (A start further left than L + k symbols cannot be
    within the budget, so the starts tried are bounded by that; empty matches never are, since k < L.)"""
    text = [int(x) for x in text]
    off = [0, len(text)] if offsets is None else [int(x) for x in offsets]
    out = []
    for w, tgt in enumerate(targets):
        sym = [int(x) for x in tgt]
        L, k = len(sym), ks[w]
        for t in range(len(off) - 1):
            lo, hi = off[t], off[t + 1]
            for e in range(lo, hi):
                best = None
                for s in range(max(lo, e + 1 - L - k), e + 2):
                    d = ed(sym, text[s:e + 1])
                    if best is None or d < best[0] or (d == best[0] and s > best[1]):
                        best = (d, s)
                if best[0] <= k:
                    out.append((pos_base + e, e - best[1] + 1, w, best[0]))
    return ordered(out)


def plant(rng, target, n_edits, stranger):
    """`target` (a list of symbols) with n_edits edit operations -- substitution, insertion and deletion in turn -- at
    places three symbols apart, never the first or the last symbol, with the symbol `stranger` (in no target) put
    in, so that two edits do not merge into one and the copy begins and ends as the target does"""
    sym = list(target)
    at = sorted((int(x) for x in rng.choice(np.arange(1, len(sym) - 1, 3), size=n_edits, replace=False)), reverse=True)
    for n, p in enumerate(at):                                            # from the back, so that the places stay
        kind = "sid"[n % 3]
        if kind == "s":
            sym[p] = stranger
        elif kind == "i":
            sym.insert(p, stranger)
        else:
            del sym[p]
    return sym
