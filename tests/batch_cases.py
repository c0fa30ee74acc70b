"""Shared by the batch-scan tests (test_batch_cpu.py, test_batch_gpu.py): the boundary set and the
expected answer of a batch, which is the ORACLE's scan of every text alone -- never the library's
own plain scan."""
import numpy as np

from oracle import pyoracle as po

KEYWORDS = [b"he", b"she", b"hers", b"s"]          # nested suffixes: "she" ends with "he", "hers" ends with "s"
# cuts inside a keyword ("us|hers", "sh|e"), right behind one ("she|"), right in front of one ("|hers"),
# with empty texts at the front, in the middle and at the end
TEXTS = [b"", b"us", b"hers and sh", b"e sells she", b"", b"", b"hers", b"xhe", b"rs", b"s", b"ushers he she hers", b"", b""]


def offsets_of(texts):
    off = np.zeros(len(texts) + 1, np.uint64)
    if len(texts):
        np.cumsum([len(t) for t in texts], out=off[1:])
    return off


def oracle_batch(o, texts):
    """(records, text_id, first) by the definition: every text alone, end_pos shifted by its offset"""
    recs, tids, first, off = [np.zeros(0, po.RECORD_DTYPE)], [np.zeros(0, np.uint32)], [0], 0
    for t, text in enumerate(texts):
        r = o.scan(text).copy() if len(text) else np.zeros(0, po.RECORD_DTYPE)
        r["end_pos"] += np.uint64(off)
        recs.append(r)
        tids.append(np.full(r.size, t, np.uint32))
        first.append(first[-1] + r.size)
        off += len(text)
    return np.concatenate(recs), np.concatenate(tids), np.array(first, np.uint64)


def oracle_batch_cut(o, text, offsets):
    """the same for one buffer and its offsets"""
    off = [int(x) for x in offsets]
    return oracle_batch(o, [text[off[t]:off[t + 1]] for t in range(len(off) - 1)])


def broken_last_pair(n):
    """(what, offsets) of n symbols cut into 1, 2 and 257 texts, each with exactly one break of the
    contract, in the LAST pair: one text -- its only pair begins with 0, so the last offset is n - 1
    (the test of the two ends, thread 0 alone); more texts -- offsets[n_texts - 1] = n + 1 lies behind
    offsets[n_texts] = n, which only the thread of pair n_texts - 1 sees: with 257 texts that is the
    first thread of a second block of 256, or the second round of a block's stride"""
    cases = [("1 text, the last not n", [0, n - 1])]
    for n_texts in (2, 257):
        off = np.linspace(0, n, n_texts + 1).astype(np.int64)
        off[-2] = n + 1
        assert off[0] == 0 and off[-1] == n and np.all(off[1:-1] >= off[:-2]) and off[-2] > off[-1]
        cases.append(("%d texts, the last pair decreasing" % n_texts, off.tolist()))
    return cases


def random_cuts(n, mean, seed=7):
    """offsets of a buffer of n symbols cut at n // mean random points; some cut points are doubled
    and tripled so that empty texts occur, also at the very front and the very end"""
    rng = np.random.default_rng(seed)
    cuts = rng.integers(0, n + 1, n // mean)
    dup = cuts[:: max(cuts.size // 50, 1)]
    off = np.sort(np.concatenate([[0, 0, 0], cuts, dup, dup[::3], [n, n]])).astype(np.uint64)
    return off


def packed_batch(n_symbols=4096, n_texts=37):
    """4 KiB over a seven-letter alphabet, cut into 37 texts: an empty first one, one of 700 symbols
    (more than a 256-symbol batch block), 34 random ones, an empty last one -- (text, offsets)"""
    rng = np.random.default_rng(75)
    text = np.frombuffer(b"hesir .", np.uint8)[rng.integers(0, 7, size=n_symbols)].copy()
    cuts = np.sort(rng.choice(np.arange(701, n_symbols), size=n_texts - 4, replace=False))
    off = np.concatenate(([0, 0, 700], cuts, [n_symbols, n_symbols])).astype(np.uint64)
    assert off.size == n_texts + 1 and off[1] == off[0] and off[-1] == off[-2] and np.all(off[1:] >= off[:-1])
    return text, off
