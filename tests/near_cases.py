"""Shared by the NEAR tests (test_near_cpu.py, test_near_gpu.py, test_near_streams_gpu.py): the expected answer,
which is always the DEFINITION of NEAR (include/acm_near.h) in plain Python over the oracle's / tests/brute.py's
record set or over the text alone -- never the library's own scan or join, and never the closed form the
library uses.  Two derivations: near() tries, for every group and end, every first symbol S downwards and
counts the distinct keywords of the records that lie wholly inside [S, e]; near_by_text() works from byte text
alone with bytes.find / bytes.endswith on slices, without records.  A group is (keyword ids, width, need)."""
import numpy as np

from oracle import pyoracle as po
from tests.pattern_cases import as_records, brute, byte_oracle, oracle_records  # noqa: F401  (the NEAR tests take them from here)

# the fixed case: a log, keywords by id, groups as (ids, width, need)
CASE_KEYWORDS = [b"he", b"she", b"his", b"hers", b"error", b"disk", b"timeout", b"sda", b"retry"]
CASE_TEXT = (b"error: disk sda timeout; retry\n"
             b"ushers: his disk error on sda, she hers\n"
             b"retry sda disk timeout error he\n"
             b"his error, her disk; timeout sda\n")
CASE_GROUPS = [
    ([4, 5], 40, 0),                              # error NEAR/40 disk: a plain pair
    ([6, 8, 7], 30, 2),                           # two of timeout, retry, sda within 30
    ([0, 1, 3], 6, 2),                            # the nested he / she / hers, width 6: `he` inside `she` counts for both
    ([5, 7], 20, 0),                              # disk and sda: they occur in both orders
    ([4, 5, 6, 7, 8], 60, 3),                     # three of five indicator terms within 60
    ([6], 5, 0),                                  # one term, and the width is below its length: nothing
    ([0, 2, 8], 10, 1),                           # need = 1: every record of the three
]
CASE_CUT = 88                                     # one cut, inside the third line


def near_groups(nearset):
    """the list of (ids, width, need) of a binding.NearSet"""
    return [([int(x) for x in nearset.terms[int(nearset.group_ptr[g]):int(nearset.group_ptr[g + 1])]], int(nearset.groups[g][0]), int(nearset.groups[g][1]))
            for g in range(nearset.n_groups)]


def _texts(n_symbols, offsets):
    return [0, n_symbols] if offsets is None else [int(x) for x in offsets]


def near(records, group_list, n_symbols, offsets=None, pos_base=0):
    """NEAR by its definition: for every group g and every end e of a record, S goes from e downwards to the
    begin of e's text and to e + 1 - width, whichever comes first; the records with a keyword of g that begin
    at S and end at or before e join those seen so far, and the first S at which they have `need` distinct
    keywords between them and one of them ends at e is S*.  The output in the total order."""
    off = _texts(n_symbols, offsets)
    recs = [(int(r["end_pos"]) - pos_base, int(r["length"]), int(r["keyword_id"])) for r in np.asarray(records)]
    ends = sorted({e for e, _, _ in recs})
    out = []
    for g, (ids, width, need) in enumerate(group_list):
        need = need or len(ids)
        by_start = {}
        for e, length, k in recs:
            if k in ids:
                by_start.setdefault(e + 1 - length, []).append((e, k))
        for e in ends:
            begin = max(off[t] for t in range(len(off) - 1) if off[t] <= e < off[t + 1])
            inside, anchored = set(), False
            for S in range(e, max(begin, e + 1 - width) - 1, -1):
                for end, k in by_start.get(S, ()):
                    if end <= e:
                        inside.add(k)
                        anchored = anchored or end == e
                if anchored and len(inside) >= need:
                    out.append((pos_base + e, e + 1 - S, g))
                    break
    return as_records(out)


def near_by_text(keywords, group_list, text, offsets=None, pos_base=0):
    """the same for byte text from the text alone: per text, group and end e the greatest S such that the slice
    text[S .. e] ends with a keyword of the group and holds at least `need` of its keywords"""
    text = bytes(text)
    off = _texts(len(text), offsets)
    out = []
    for g, (ids, width, need) in enumerate(group_list):
        need = need or len(ids)
        words = [bytes(keywords[k]) for k in ids]
        for t in range(len(off) - 1):
            sub = text[off[t]:off[t + 1]]
            for e in range(len(sub)):
                for S in range(e, max(0, e + 1 - width) - 1, -1):
                    window = sub[S:e + 1]
                    if any(window.endswith(w) for w in words) and sum(window.find(w) >= 0 for w in words) >= need:
                        out.append((pos_base + off[t] + e, e + 1 - S, g))
                        break
    return as_records(out)


def random_case(rng):
    """(keywords, groups, text, offsets) of the random check: 1 to 5 distinct keywords of 1 to 3 symbols over
    {a, b}, 1 to 4 groups of 1 to all of them with width 1 to 12 and need 0 to m, a text of 0 to 40 symbols over
    {a, b} cut into 1 to 4 texts (empty texts included)"""
    ab = np.frombuffer(b"ab", np.uint8)
    keywords = []
    for _ in range(int(rng.integers(1, 6))):
        kw = bytes(rng.choice(ab, size=int(rng.integers(1, 4))))
        if kw not in keywords:
            keywords.append(kw)
    group_list = []
    for _ in range(int(rng.integers(1, 5))):
        m = int(rng.integers(1, len(keywords) + 1))
        ids = [int(x) for x in rng.permutation(len(keywords))[:m]]
        group_list.append((ids, int(rng.integers(1, 13)), int(rng.integers(0, m + 1))))
    n = int(rng.integers(0, 41))
    text = bytes(rng.choice(ab, size=n))
    cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 4))))
    offsets = np.array([0] + [int(c) for c in cuts] + [n], np.uint64)
    return keywords, group_list, text, offsets


def random_cases(n=300, seed=1975):
    """the n seeded random cases with their answers, computed once per process: a list of (keywords, groups,
    text, offsets, records, want)"""
    if (n, seed) not in _RANDOM:
        rng = np.random.default_rng(seed)
        cases = []
        for _ in range(n):
            kws, group_list, text, offsets = random_case(rng)
            rec = oracle_records(kws, text)
            cases.append((kws, group_list, text, offsets, rec, near(rec, group_list, len(text), offsets)))
        _RANDOM[(n, seed)] = cases
    return _RANDOM[(n, seed)]


_RANDOM = {}


def case_facts(keywords, group_list, text, cut):
    """what makes the fixed case worth running, from the definition alone: (matches per group, ties in end_pos,
    matches at whose end two records of the group end -- two anchors --, those of them whose window begins with
    an anchor that is not the nearest one (the shortest record that ends there), matches lost to one cut)"""
    rec = oracle_records(keywords, text)
    want = near(rec, group_list, len(text))
    per = np.bincount(want["keyword_id"], minlength=len(group_list)).tolist()
    ties = int(np.count_nonzero(want["end_pos"][1:] == want["end_pos"][:-1]))
    two = far = 0
    for r in want:
        e, S, ids = int(r["end_pos"]), int(r["end_pos"]) + 1 - int(r["length"]), group_list[int(r["keyword_id"])][0]
        starts = sorted(e + 1 - len(keywords[k]) for k in ids if text[:e + 1].endswith(keywords[k]))
        two += len(starts) >= 2
        far += len(starts) >= 2 and S in starts[:-1]
    lost = want.size - near(rec, group_list, len(text), [0, cut, len(text)]).size
    return per, ties, two, far, lost
