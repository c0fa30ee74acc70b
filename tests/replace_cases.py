"""Shared by the replace tests (test_replace_cpu.py, test_replace_gpu.py): the expected answer, which is
always the definition of REPLACE (include/acm_gpu.h) in plain Python, applied to select_cases.greedy
over the ORACLE's records -- never the library's own scan or selection --, and the check that a case
cannot pass trivially."""
import numpy as np

from tests.select_cases import greedy, oracle_records


def as_symbols(x, dtype=np.uint8):
    if isinstance(x, (bytes, bytearray)):
        x = np.frombuffer(bytes(x), np.uint8)
    return np.asarray(x).astype(dtype).reshape(-1)


def replace_by_definition(text, sel, replacements=None, fill=None, pos_base=0):
    """(REPLACE (text, sel, table) as an array of text's dtype, out_start as int64): the pieces of the
    definition laid end to end; out_start once more by its formula, and the two agree"""
    t = as_symbols(text, np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text).reshape(-1)
    parts, starts, at, nxt = [], [], 0, 0
    grown = []
    for r in sel:
        e = int(r["end_pos"]) - pos_base
        s = e + 1 - int(r["length"])
        assert nxt <= s and e < t.size
        parts.append(t[nxt:s])
        at += s - nxt
        starts.append(at)
        rep = (np.full(int(r["length"]), fill, t.dtype) if replacements is None else as_symbols(replacements[int(r["keyword_id"])], t.dtype))
        parts.append(rep)
        at += rep.size
        grown.append(rep.size - int(r["length"]))
        nxt = e + 1
    parts.append(t[nxt:])
    out = np.concatenate(parts).astype(t.dtype)
    starts = np.array(starts, np.int64)
    s_j = sel["end_pos"].astype(np.int64) + 1 - sel["length"].astype(np.int64) - pos_base
    formula = s_j + np.concatenate([[0], np.cumsum(np.array(grown, np.int64))[:-1]]) if len(sel) else np.zeros(0, np.int64)
    assert np.array_equal(starts, formula)
    return out, starts


def oracle_case(o, text, replacements=None, fill=None):
    """(all records, selection, expected output, expected out_start) from the oracle alone, shown to be
    no trivial case: a record is selected, a record is left out, the output differs from the input"""
    rec = oracle_records(o, text)
    sel = greedy(rec)
    want, starts = replace_by_definition(text, sel, replacements, fill)
    t = as_symbols(text, want.dtype)
    print("records %d, selected %d, symbols %d -> %d" % (rec.size, sel.size, t.size, want.size))
    assert 0 < sel.size < rec.size, (sel.size, rec.size)
    assert want.size != t.size or not np.array_equal(want, t)
    return rec, sel, want, starts


def random_table(rng, n_keywords, lo=0, hi=5, alphabet=(65, 91), dtype=np.uint8):
    """replacements of lo .. hi symbols over another alphabet than the texts' (A-Z)"""
    return [rng.integers(alphabet[0], alphabet[1], size=int(rng.integers(lo, hi + 1))).astype(dtype) for _ in range(n_keywords)]
