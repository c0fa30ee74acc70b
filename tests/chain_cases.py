"""Shared by the chain tests (test_chains_cpu.py, test_chains_gpu.py): the expected answer, which is always the
DEFINITION of CHAINS (include/acm_gpu.h) in plain Python over the oracle's / tests/brute.py's record set --
never the library's own scan or join.  Two derivations that share nothing with the library's dynamic
programme over "the best start": chains() enumerates, per record and level, EVERY first-symbol position of an
embedding that ends there (a set, kept as the bits of a Python integer) and tests the text on every one of
them; chains_by_re() works from byte text alone with `re` (`A.{min,max}B`, for every end the latest start
whose slice matches in full, per text)."""
import bisect
import re

import numpy as np

from oracle import pyoracle as po
from tests.pattern_cases import as_records, brute, byte_oracle, oracle_records  # noqa: F401  (the chain tests take them from here)

# the fixed case of the GPU tests: a log of requests, keywords by id, chains as [kw, (min, max), kw, ...] over the ids
CASE_KEYWORDS = [b"GET", b"HTTP", b"Host", b"/", b"1.1", b":", b"id="]
CASE_TEXT = (b"GET /a/b?id=7 HTTP/1.1 Host: x:80 GET /c HTTP/1.1 Host: y id=9 GET /id=3/x HTTP/1.0 Host: z "
             b"GET / HTTP/1.1 Host:: id=1 /1.1")
CASE_CHAINS = [
    [(0, 0, 0), (1, 2, 40)],                      # GET .{2,40} HTTP: two GETs reach some HTTP -- the latest start is not the earliest
    [(3, 0, 0), (6, 0, 3), (1, 1, 12)],           # / .{0,3} id= .{1,12} HTTP: a later `/` has no id= behind it -- the middle gap rules it out
    [(3, 0, 0), (4, 0, 0)],                       # `/` then `1.1` at once: a fixed gap of 0
    [(1, 0, 0), (3, 0, 0), (4, 0, 0)],            # HTTP/1.1
    [(2, 0, 0), (5, 0, 1), (5, 0, 4)],            # Host :{0,1} then another `:` within 4
    [(6, 0, 0), (4, 2, 24)],                      # id= .{2,24} 1.1: ends where chains 2 and 3 end
]
CASE_CUT = 40                                     # one cut, inside the first request's reach


def chain_terms(chainset):
    """the lists of (keyword_id, gap_min, gap_max) of a binding.ChainSet"""
    return [[tuple(int(x) for x in chainset.terms[i]) for i in range(int(chainset.chain_ptr[c]), int(chainset.chain_ptr[c + 1]))]
            for c in range(chainset.n_chains)]


def embeddings(records, chain_list, pos_base=0):
    """per chain a list of (e, starts) over the records that can end it: `starts` has bit s set iff an
    embedding of the chain that ends in this record begins at buffer index s.  Exhaustive: nothing is
    dropped on the way, whatever the texts are."""
    recs = [(int(r["end_pos"]) - pos_base, int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)]
    ends = [e for e, _, _ in recs]
    out = []
    for terms in chain_list:
        reach = [0] * len(recs)
        for j, (k, gmin, gmax) in enumerate(terms):
            new = [0] * len(recs)
            for i, (e, length, kk) in enumerate(recs):
                if kk != k:
                    continue
                s = e + 1 - length
                if j == 0:
                    new[i] = 1 << s
                    continue
                lo, hi = s - 1 - gmax, s - 1 - gmin
                if hi < 0:
                    continue
                acc = 0
                for w in range(bisect.bisect_left(ends, max(lo, 0)), bisect.bisect_right(ends, hi)):
                    if recs[w][2] == terms[j - 1][0]:
                        acc |= reach[w]
                new[i] = acc
            reach = new
        out.append([(recs[i][0], reach[i]) for i in range(len(recs)) if reach[i]])
    return out


def chains(records, chain_list, n_symbols, offsets=None, pos_base=0):
    """CHAINS by its definition: for every chain c and end e the greatest s_0 among the embeddings of c that end
    at e and whose s_0 lies in the text of e; the output in the total order"""
    off = [0, n_symbols] if offsets is None else [int(x) for x in offsets]
    out = []
    for c, per_end in enumerate(embeddings(records, chain_list, pos_base)):
        for e, starts in per_end:
            for t in range(len(off) - 1):
                if off[t] <= e < off[t + 1]:
                    inside = starts & ((1 << (e + 1)) - (1 << off[t]))       # the starts in [off[t], e]
                    if inside:
                        out.append((pos_base + e, e + 1 - (inside.bit_length() - 1), c))
    return as_records(out)


def chains_by_re(keywords, chain_list, text, offsets=None, pos_base=0):
    """the same for byte text from the text alone: per text, chain and end the latest start S such that
    text[S .. e] is, in full, the chain's keywords with min to max arbitrary bytes between them"""
    text = bytes(text)
    off = [0, len(text)] if offsets is None else [int(x) for x in offsets]
    out = []
    for c, terms in enumerate(chain_list):
        rx = re.compile(b"".join((b".{%d,%d}" % (gmin, gmax) if j else b"") + re.escape(bytes(keywords[k])) for j, (k, gmin, gmax) in enumerate(terms)),
                        re.S)
        shortest = sum(len(keywords[k]) + gmin for k, gmin, _ in terms)
        longest = sum(len(keywords[k]) + gmax for k, _, gmax in terms)
        for t in range(len(off) - 1):
            sub = text[off[t]:off[t + 1]]
            for e in range(shortest - 1, len(sub)):
                for S in range(e + 1 - shortest, max(e - longest, -1), -1):
                    if rx.fullmatch(sub, S, e + 1):
                        out.append((pos_base + off[t] + e, e + 1 - S, c))
                        break
    return as_records(out)


def fixed_offset_patterns(keywords, chain_list):
    """the PATTERNS terms (keyword_id, offset, length) of chains whose gaps all have gap_min == gap_max"""
    pats = []
    for terms in chain_list:
        at, pat = 0, []
        for k, gmin, gmax in terms:
            assert gmin == gmax
            at += gmin
            pat.append((k, at, len(keywords[k])))
            at += len(keywords[k])
        pats.append(pat)
    return pats


def random_case(rng):
    """(keywords, chains, text, offsets) of the random check: 1 to 4 distinct keywords of 1 to 3 symbols over
    {a, b}, 1 to 4 chains of 1 to 4 terms with gap_min 0 to 3 and gap_max up to gap_min + 4, a text of 0 to 40
    symbols over {a, b} cut into 1 to 4 texts (empty texts included)"""
    ab = np.frombuffer(b"ab", np.uint8)
    keywords = []
    for _ in range(int(rng.integers(1, 5))):
        kw = bytes(rng.choice(ab, size=int(rng.integers(1, 4))))
        if kw not in keywords:
            keywords.append(kw)
    chain_list = []
    for _ in range(int(rng.integers(1, 5))):
        terms = []
        for j in range(int(rng.integers(1, 5))):
            gmin = int(rng.integers(0, 4)) if j else 0
            terms.append((int(rng.integers(0, len(keywords))), gmin, gmin + int(rng.integers(0, 5)) if j else 0))
        chain_list.append(terms)
    n = int(rng.integers(0, 41))
    text = bytes(rng.choice(ab, size=n))
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 4))))
    offsets = np.array([0] + [int(c) for c in cuts] + [n], np.uint64)
    return keywords, chain_list, text, offsets


def case_facts(keywords, chain_list, text, cut):
    """what makes the fixed case worth running, from the definition alone: (matches per chain, ties in end_pos,
    ends whose latest start is not their earliest, matches whose nearest first keyword is not the start
    because a gap in the middle rules it out, matches lost to one cut)"""
    rec = oracle_records(keywords, text)
    want = chains(rec, chain_list, len(text))
    per = np.bincount(want["keyword_id"], minlength=len(chain_list)).tolist()
    ties = int(np.count_nonzero(want["end_pos"][1:] == want["end_pos"][:-1]))
    several = sum(1 for per_end in embeddings(rec, chain_list) for _, starts in per_end if starts & (starts - 1))
    ruled_out = 0
    for r in want:
        e, S, terms = int(r["end_pos"]), int(r["end_pos"]) + 1 - int(r["length"]), chain_list[int(r["keyword_id"])]
        if len(terms) < 3:
            continue
        last_start = e + 1 - len(keywords[terms[-1][0]])
        first = keywords[terms[0][0]]
        ruled_out += any(text[s:s + len(first)] == first for s in range(S + 1, last_start - len(first) + 1))
    lost = want.size - chains(rec, chain_list, len(text), [0, cut, len(text)]).size
    return per, ties, several, ruled_out, lost
