"""Shared by the anchored-match tests (test_anchored_cpu.py, test_anchored_gpu.py): the expected answer,
which is always the DEFINITION of ANCHORED and LOOKUP (include/acm_gpu.h) in plain Python over the
ORACLE's records -- never the library's own scan or filter --, the hand-made batch with its table of
literals, and the cut maker that turns a buffer and its oracle records into a batch whose anchored
records are known to be many."""
import numpy as np

from oracle import pyoracle as po
from tests.batch_cases import offsets_of, oracle_batch

PREFIXES, LONGEST, WHOLE = 1, 2, 3
MODES = (PREFIXES, LONGEST, WHOLE)
NONE = 0xFFFFFFFF

# ---- the hand-made batch
KEYWORDS = [b"h", b"he", b"her", b"hers", b"hershey", b"she", b"his"]
TEXTS = [b"", b"h", b"he", b"her", b"hers", b"hershey", b"hersheys", b"hex", b"she", b"xhe", b"s", b"ushers", b"he", b"rs", b"", b"hers"]
# "hersheys": five prefixes and no whole; "hex": two; "ushers": five matches of the batch scan and none anchored;
# "he" | "rs": no `her`, no `hers` across the cut; the last text ends at n_symbols
PREFIX_COUNTS = [0, 1, 2, 3, 4, 5, 5, 2, 1, 0, 0, 0, 2, 0, 0, 4]
WHOLE_TEXTS = [1, 2, 3, 4, 5, 8, 12, 15]
N_PREFIXES = sum(PREFIX_COUNTS)                          # 29 records


def batch_records(o, text, offsets):
    """(records, text of each) of acm_scan_batch by ONE oracle scan of the packed buffer: the batch's
    records are exactly the buffer's that lie inside one text (include/acm_gpu.h, batch scan)"""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    rec = o.scan(text) if len(text) else np.zeros(0, po.RECORD_DTYPE)
    end = rec["end_pos"].astype(np.int64)
    start = end + 1 - rec["length"].astype(np.int64)
    t = np.searchsorted(off, start, side="right") - 1       # the text with off[t] <= start < off[t + 1]
    inside = end < off[t + 1]
    return rec[inside], t[inside]


def anchored(records, offsets, mode, text_of=None):
    """ANCHORED (B, offsets, mode) by its definition: `records` is B in canonical order.  Returns
    (records, text_id, first)."""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    n_texts = off.size - 1
    rec = np.asarray(records)
    end = rec["end_pos"].astype(np.int64)
    length = rec["length"].astype(np.int64)
    start = end + 1 - length
    t = np.searchsorted(off, start, side="right") - 1 if text_of is None else np.asarray(text_of, np.int64)
    assert np.all(off[t] <= start) and np.all(end < off[t + 1])
    keep = start == off[t]                                   # P_t: the records of text t that begin where it begins
    if mode == WHOLE:
        keep &= length == off[t + 1] - off[t]
    idx = np.flatnonzero(keep)
    if mode == LONGEST and idx.size:                         # the last of every text's run (ascending length inside a text)
        last = np.ones(idx.size, bool)
        last[:-1] = t[idx][1:] != t[idx][:-1]
        idx = idx[last]
    out, tid = rec[idx].astype(po.RECORD_DTYPE), t[idx].astype(np.uint32)
    assert np.all(np.diff(tid.astype(np.int64)) >= 0) and np.all(np.diff(out["end_pos"].astype(np.int64)) > 0)
    first = np.searchsorted(tid, np.arange(n_texts + 1), side="left").astype(np.uint64)
    return out, tid, first


def lookup(records, offsets, text_of=None):
    """LOOKUP by its definition: (whole_id, prefix_id, prefix_len), one entry per text"""
    n_texts = len(offsets) - 1
    whole_id, prefix_id, prefix_len = np.full(n_texts, NONE, np.uint32), np.full(n_texts, NONE, np.uint32), np.zeros(n_texts, np.uint32)
    rec, tid, _ = anchored(records, offsets, WHOLE, text_of)
    whole_id[tid] = rec["keyword_id"]
    rec, tid, _ = anchored(records, offsets, LONGEST, text_of)
    prefix_id[tid] = rec["keyword_id"]
    prefix_len[tid] = rec["length"]
    return whole_id, prefix_id, prefix_len


def expected(o, text, offsets):
    """everything a test compares against, computed once: {mode: (records, text_id, first)} and the lookup arrays"""
    rec, t = batch_records(o, text, offsets)
    return {m: anchored(rec, offsets, m, t) for m in MODES}, lookup(rec, offsets, t)


def hand_made(o):
    """(packed text, offsets, expected) of the hand-made batch; the table's literals are asserted
    against the oracle-derived answer first, so that the table itself is checked"""
    off = offsets_of(TEXTS)
    packed = b"".join(TEXTS)
    rec, tid, first = oracle_batch(o, TEXTS)
    want = {m: anchored(rec, off, m, tid) for m in MODES}
    look = lookup(rec, off, tid)
    counts = np.diff(want[PREFIXES][2].astype(np.int64))
    assert counts.tolist() == PREFIX_COUNTS and int(counts.sum()) == N_PREFIXES
    assert want[WHOLE][1].tolist() == WHOLE_TEXTS and np.flatnonzero(look[0] != NONE).tolist() == WHOLE_TEXTS
    assert int(np.count_nonzero(tid == 11)) == 5 and counts[11] == 0          # "ushers": she, h, he, her, hers -- none anchored
    assert set(rec["keyword_id"][tid == 12].tolist()) == {0, 1} and not np.any(tid == 13)  # "he" | "rs"
    assert int(off[-1]) == len(packed) and counts[15] == 4
    # LONGEST of "hersheys" is hershey, of "hex" is he
    assert (look[1][6], look[2][6], look[1][7], look[2][7]) == (4, 7, 1, 2)
    # both derivations of a batch's records agree
    rec1, t1 = batch_records(o, packed, off)
    assert np.array_equal(rec1, rec) and np.array_equal(t1, tid)
    return packed, off, want, look


def plant(text, records, every=256, seed=75):
    """a copy of `text` (an array of symbols) with the spelling of one of its own matches, drawn at random
    from `records`, written at every `every`-th symbol: a text of few matches becomes one of thousands"""
    rng = np.random.default_rng(seed)
    out = np.array(text, copy=True)
    rec = np.asarray(records)
    for p in range(every // 2, out.size - 64, every):
        r = rec[int(rng.integers(0, rec.size))]
        e, length = int(r["end_pos"]), int(r["length"])
        if length <= 64:
            out[p:p + length] = text[e + 1 - length:e + 1]
    return out


def make_cuts(n, records, seed=1975, n_chosen=3000, n_random=3000, must=()):
    """offsets[] of a buffer of n symbols from its oracle records: records with pairwise disjoint spans
    at least 64 symbols apart are chosen (those of the keyword ids in `must` first), a cut goes to the
    start of each and, for every second one, to its end + 1; random cuts that fall inside no chosen
    span are added, and some cuts are doubled so that empty texts exist.  By construction every
    chosen record is anchored and every second one spells its whole text.  Returns (offsets, chosen records)."""
    rng = np.random.default_rng(seed)
    rec = np.asarray(records)
    end = rec["end_pos"].astype(np.int64)
    start = end + 1 - rec["length"].astype(np.int64)
    forced = [int(np.flatnonzero(rec["keyword_id"] == k)[0]) for k in must]
    taken = np.zeros(n + 129, bool)                          # symbols within 64 of a chosen span
    chosen = []
    for j in forced + list(range(rec.size)):                 # earliest end first: the most spans that fit
        s, e = int(start[j]), int(end[j])
        if np.any(taken[s + 64:e + 65]):
            continue
        taken[s:e + 129] = True                              # [s - 64, e + 64], shifted by 64
        chosen.append(int(j))
    if len(chosen) > n_chosen:                               # a random subset of them, the forced ones among it
        rest = np.array(chosen[len(forced):], np.int64)
        chosen = forced + [int(j) for j in rest[rng.permutation(rest.size)[:n_chosen - len(forced)]]]
    chosen = np.array(sorted(chosen, key=lambda j: start[j]), np.int64)
    cuts = list(start[chosen]) + list(end[chosen[::2]] + 1)
    inside = np.zeros(n + 2, bool)                           # a cut at p is inside a span when start < p <= end
    for j in chosen:
        inside[start[j] + 1:end[j] + 1] = True
    more = rng.integers(0, n + 1, n_random)
    more = more[~inside[more]]
    cuts = np.concatenate([np.array(cuts, np.int64), more])
    dup = cuts[rng.permutation(cuts.size)[: max(cuts.size // 20, 2)]]
    off = np.sort(np.concatenate([[0, 0], cuts, dup, [n, n]])).astype(np.uint64)
    return off, rec[chosen]


def nontrivial(want, look, chosen=None, many=True):
    """from the oracle's answer alone: the batch cannot pass trivially"""
    counts = np.diff(want[PREFIXES][2].astype(np.int64))
    with_prefix, with_whole, none, nested = (int(np.count_nonzero(counts > 0)), int(np.count_nonzero(look[0] != NONE)),
                                             int(np.count_nonzero(counts == 0)), int(np.count_nonzero(counts >= 2)))
    print("texts %d: with a prefix %d, whole %d, none %d, two or more prefixes %d; records %d" % (counts.size, with_prefix, with_whole, none, nested,
                                                                                               int(counts.sum())))
    if many:
        assert with_prefix >= 1000 and with_whole >= 400 and none >= 1000, (with_prefix, with_whole, none)
    if chosen is not None:                                   # by construction: every chosen record is anchored, every second one whole
        got = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in want[PREFIXES][0]}
        assert all((int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) in got for r in chosen)
        whole = {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in want[WHOLE][0]}
        assert all((int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) in whole for r in chosen[::2])
    return with_prefix, with_whole, none, nested


def novel_batch(novel_bytes, n_chosen=3000, n_random=3000):
    """(keywords, oracle, text, offsets, expected, lookup) of the novel under the dictionary of its own
    words (the / them / then / there ...): at least 100 texts begin with two or more keywords"""
    from tests.tally_cases import byte_oracle, novel_words
    keywords = novel_words(novel_bytes)
    o = byte_oracle(keywords)
    rec = o.scan(novel_bytes)
    off, chosen = make_cuts(len(novel_bytes), rec, n_chosen=n_chosen, n_random=n_random)
    want, look = expected(o, novel_bytes, off)
    nested = nontrivial(want, look, chosen)[3]
    assert nested >= 100, nested
    return keywords, o, novel_bytes, off, want, look
