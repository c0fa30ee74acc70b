"""Shared by the tokenising tests (test_tokens_cpu.py, test_tokens_gpu.py): the expected answer, which is
always the definition of the token stream (include/acm_gpu.h) in plain Python, applied to
select_cases.greedy over the ORACLE's records -- per text via batch_cases.oracle_batch for batches,
never the library's own scan or selection --, and the check that a case cannot pass trivially."""
import numpy as np

from oracle import pyoracle as po
from tests.batch_cases import oracle_batch
from tests.select_cases import greedy, oracle_records

SYMBOL, RUN, DROP = 0, 1, 2
MODES = [SYMBOL, RUN, DROP]


def as_symbols(text):
    if isinstance(text, (bytes, bytearray)):
        return np.frombuffer(bytes(text), np.uint8)
    return np.asarray(text).reshape(-1)


def tokens_by_definition(text, sel, mode, gap_base=0, tok_of=None, offsets=None, pos_base=0):
    """(ids uint32, starts uint64, lengths uint32, first uint64 or None): symbol by symbol.  A symbol is
    covered when a selected record holds it; a match is a unit, and by mode every uncovered symbol
    (SYMBOL), every maximal run of uncovered symbols inside one text (RUN) or nothing else (DROP).
    first[t] = the number of tokens that begin in front of offsets[t]."""
    t = as_symbols(text)
    n = t.size
    owner = np.full(n, -1, np.int64)                       # the record that covers symbol i
    for j, r in enumerate(sel):
        e = int(r["end_pos"]) - pos_base
        s = e + 1 - int(r["length"])
        assert 0 <= s <= e < n and np.all(owner[s:e + 1] == -1)
        owner[s:e + 1] = j
    text_start = np.zeros(n + 1, bool)
    if offsets is not None:
        off = [int(x) for x in offsets]
        assert off[0] == 0 and off[-1] == n and all(a <= b for a, b in zip(off, off[1:]))
        text_start[off] = True
    ids, starts, lens = [], [], []
    i = 0
    while i < n:
        j = int(owner[i])
        if j >= 0:                                          # a match: it begins here (records never overlap)
            kw = int(sel[j]["keyword_id"])
            ids.append(int(tok_of[kw]) if tok_of is not None else kw)
            starts.append(i)
            lens.append(int(sel[j]["length"]))
            if offsets is not None:                         # no record crosses a text boundary
                assert not np.any(text_start[i + 1:i + lens[-1]])
            i += lens[-1]
        elif mode == SYMBOL:
            ids.append((gap_base + int(t[i])) & 0xFFFFFFFF)
            starts.append(i)
            lens.append(1)
            i += 1
        elif mode == RUN:
            k = i + 1
            while k < n and owner[k] < 0 and not text_start[k]:
                k += 1
            ids.append(gap_base)
            starts.append(i)
            lens.append(k - i)
            i = k
        else:
            i += 1
    starts = np.array(starts, np.int64)
    first = None
    if offsets is not None:
        first = np.array([np.count_nonzero(starts < o) for o in off], np.uint64) if len(off) < 4096 else np.searchsorted(
            starts, np.array(off, np.int64), side="left").astype(np.uint64)
    return np.array(ids, np.uint32), (starts + pos_base).astype(np.uint64), np.array(lens, np.uint32), first


def selection_of(o, text, offsets=None):
    """(all records, the selection) from the oracle: of one text, or per text of a batch (oracle_batch)"""
    t = as_symbols(text)
    if offsets is None:
        rec = oracle_records(o, t)
        return rec, greedy(rec)
    off = [int(x) for x in offsets]
    rec, _, first = oracle_batch(o, [t[off[k]:off[k + 1]] for k in range(len(off) - 1)])
    parts = [greedy(rec[int(first[k]):int(first[k + 1])]) for k in range(len(off) - 1)]
    return rec, (np.concatenate(parts) if parts else np.zeros(0, po.RECORD_DTYPE)).astype(po.RECORD_DTYPE)


def nontrivial(text, rec, sel, offsets=None):
    """from the oracle alone: a record is selected, a record is left out, a gap token exists; for a
    batch a run of uncovered symbols is cut by a text boundary and a text is empty"""
    n = as_symbols(text).size
    covered = int(sel["length"].astype(np.int64).sum())
    print("symbols %d, records %d, selected %d, covered %d" % (n, rec.size, sel.size, covered))
    assert 0 < sel.size < rec.size, (sel.size, rec.size)
    assert covered < n
    if offsets is not None:
        off = np.asarray(offsets, np.int64)
        assert np.any(off[1:] == off[:-1]), "no empty text"
        unc = np.ones(n, bool)
        for r in sel:
            e = int(r["end_pos"])
            unc[e + 1 - int(r["length"]):e + 1] = False
        inner = off[(off > 0) & (off < n)]
        assert np.any(unc[inner] & unc[inner - 1]), "no run is cut by a text boundary"


def oracle_case(o, text, offsets=None):
    """(all records, selection) of a workload case, shown to be no trivial one"""
    rec, sel = selection_of(o, text, offsets)
    nontrivial(text, rec, sel, offsets)
    return rec, sel
