"""Shared by the flow-scan tests (test_flows_cpu.py, test_flows_gpu.py): scenarios of calls whose
texts continue earlier ones, and their expected answer -- which comes from the ORACLE alone: every
flow's whole history is scanned once with Oracle.scan, its records are sliced by the range of end
positions of each piece and rebased to the piece's offset in its call's buffer.  Never the library's
own plain or batch scan."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from oracle import pyoracle as po
from tests.batch_cases import offsets_of, oracle_batch

EMPTY = np.zeros(0, po.RECORD_DTYPE)


class Call:
    """one flow call: texts[t] (arrays of symbols) continues flow flows[t]"""

    def __init__(self, texts, flows):
        self.texts = [np.frombuffer(t, np.uint8) if isinstance(t, (bytes, bytearray)) else np.asarray(t) for t in texts]
        self.flows = [int(f) for f in flows]
        assert len(self.texts) == len(self.flows) and len(set(self.flows)) == len(self.flows)
        self.offsets = offsets_of(self.texts)

    def buffer(self, dtype):
        return np.concatenate([np.zeros(0, dtype)] + [t.astype(dtype, copy=False) for t in self.texts])


class Reset:
    """between two calls: these flows go back to the root (None: all)"""

    def __init__(self, flows=None):
        self.flows = None if flows is None else [int(f) for f in flows]


def expected(o, steps, dtype=np.uint8):
    """per Call of `steps` (Reset entries are skipped in the result): (records, text_id, first)"""
    pieces = {}                                  # flow -> [(call index, text index, begin, end)] of its current history
    history = {}                                 # flow -> [arrays]
    per_piece = {}                               # (call index, text index) -> records with end_pos inside the piece

    def close(f):
        if f not in history:
            return
        whole = np.concatenate([np.zeros(0, dtype)] + [h.astype(dtype, copy=False) for h in history.pop(f)])
        rec = o.scan(whole) if whole.size else EMPTY
        ends = rec["end_pos"]
        for (i, t, a, b) in pieces.pop(f):
            lo, hi = np.searchsorted(ends, [a, b])
            r = rec[lo:hi].copy()
            r["end_pos"] -= np.uint64(a)
            per_piece[(i, t)] = r

    for i, step in enumerate(steps):
        if isinstance(step, Reset):
            for f in (list(history) if step.flows is None else step.flows):
                close(f)
            continue
        for t, (text, f) in enumerate(zip(step.texts, step.flows)):
            seen = sum(h.size for h in history.get(f, []))
            history.setdefault(f, []).append(text)
            pieces.setdefault(f, []).append((i, t, seen, seen + text.size))
    for f in list(history):
        close(f)
    out = []
    for i, step in enumerate(steps):
        if isinstance(step, Reset):
            continue
        recs, tids, first = [EMPTY], [np.zeros(0, np.uint32)], [0]
        for t in range(len(step.texts)):
            r = per_piece[(i, t)]
            r["end_pos"] += step.offsets[t]
            recs.append(r)
            tids.append(np.full(r.size, t, np.uint32))
            first.append(first[-1] + r.size)
        out.append((np.concatenate(recs), np.concatenate(tids), np.array(first, np.uint64)))
    return out


def nontrivial(o, steps, want, dtype=np.uint8, every_call=False):
    """from the oracle alone: the flow answer has strictly more records than the batch answer of the
    same texts (matches across a cut exist), and it is not the scan of a call's buffer as one text
    (neighbouring texts of different flows must not join).  every_call: every call BEHIND THE FIRST
    must differ from its concatenation -- in the first call of a scenario all flows are at the root,
    the flow answer is the batch answer, and whether the concatenation has a match across two
    neighbouring texts there is chance; the later calls carry symbols over, which the concatenation
    cannot know"""
    calls = [s for s in steps if isinstance(s, Call)]
    flow_total = sum(w[0].size for w in want)
    batch_total = sum(oracle_batch(o, c.texts)[0].size for c in calls)
    differs = []
    for c, w in zip(calls, want):
        buf = c.buffer(dtype)
        whole = o.scan(buf) if buf.size else EMPTY
        differs.append(not (whole.size == w[0].size and np.array_equal(whole, w[0])))
    print("flow records %d, batch records %d, calls that differ from their concatenation %d of %d" % (
        flow_total, batch_total, sum(differs), len(differs)))
    assert flow_total > batch_total, (flow_total, batch_total)
    assert any(differs) and (all(differs[1:]) or not every_call), differs


# ---- the boundary set: keywords he, she, hers, s (the carry is 3 symbols), five flows over four calls
KEYWORDS = [b"he", b"she", b"hers", b"s"]
N_FLOWS = 300
A, B, Cc, D, E = 299, 0, 17, 150, 42              # sparse, permuted ids


def boundary_steps():
    return [
        # cut inside a keyword ("us|hers", "sh|e"), a one-symbol piece, an empty piece; flow E is absent
        Call([b"us", b"and sh", b"h", b""], [A, B, Cc, D]),
        # flow C's carry is assembled from three one-symbol pieces ("h" above, "e", "r", then "s...")
        Call([b"e", b"hers she", b"e sells", b"xs"], [Cc, A, B, E]),
        Call([b"r", b"", b"he", b"h"], [Cc, A, D, E]),
        Call([b"s and ushers", b"rs", b"ers", b"", b"he"], [Cc, D, E, B, A]),
    ]


def identity_steps():
    """d_flow = NULL: text t is flow t"""
    return [Call([b"ush", b"s", b"", b"he"], [0, 1, 2, 3]), Call([b"ers", b"he", b"hers", b"rs"], [0, 1, 2, 3])]


def deal(text, offsets, n_flows, n_calls, seed=11):
    """the pieces text[offsets[k] : offsets[k + 1]] as n_calls Calls: n_calls consecutive pieces are one
    flow's stream (so every cut inside a stream is one that a keyword may lie across), call c holds
    piece c of every stream, in random order, and the streams get flow ids drawn at random without
    repeats"""
    rng = np.random.default_rng(seed)
    off = [int(x) for x in offsets]
    n_pieces = len(off) - 1
    n_streams = (n_pieces + n_calls - 1) // n_calls
    assert n_streams <= n_flows, (n_streams, n_flows)
    ids = rng.permutation(n_flows)[:n_streams]
    calls = []
    for c in range(n_calls):
        js = [int(j) for j in rng.permutation(n_streams) if j * n_calls + c < n_pieces]
        calls.append(Call([text[off[j * n_calls + c]:off[j * n_calls + c + 1]] for j in js], [ids[j] for j in js]))
    return calls


# ---- a machine the GPU cannot take: ACM_CMP_DEFAULT over 3-byte symbols (the host loop)
def sym3(word):
    """bytes -> the same word in 3-byte symbols (as bytes): the letter c is (c, c ^ 0x5A, 7)"""
    w = np.frombuffer(bytes(word), np.uint8)
    return np.stack([w, w ^ 0x5A, np.full_like(w, 7)], axis=1).tobytes()


def raw_machine3(keywords):
    L = acm.lib()
    arg = C.c_size_t(3)
    keep = [arg]
    h = L.acm_create(C.c_void_p.in_dll(L, "ACM_CMP_DEFAULT"), C.cast(C.pointer(arg), C.c_void_p), None)
    for kw in keywords:
        buf = np.frombuffer(sym3(kw), dtype=np.uint8).copy()
        keep.append(buf)
        cur = C.c_void_p(L.acm_initiate(h))
        for i in range(len(kw)):
            L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + i * 3)
        L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    return h, keep


def split_scan(L, handle, text, sym_bytes, a, b, counts, want, cap=None):
    """the caller's cursor over text[:a] symbol by symbol (acm_match), text[a:b] in one acm_scan_from,
    text[b:] symbol by symbol again.  `counts[i]` = matches ending at symbol i and `want` = the
    records of the ORACLE's single loop over the whole text.  Checks all three parts."""
    from aho_corasick_1975_amd import binding
    buf = np.frombuffer(bytes(text), np.uint8).copy() if not isinstance(text, np.ndarray) else np.ascontiguousarray(text)
    base = buf.ctypes.data
    n = buf.size * buf.itemsize // sym_bytes
    cur = C.c_void_p(L.acm_initiate(handle))
    for i in range(a):
        assert L.acm_match(C.byref(cur), base + i * sym_bytes) == counts[i], ("prefix", a, b, i)
    lo, hi = np.searchsorted(want["end_pos"], [a, b])
    need = hi - lo
    rec = np.zeros(max(need, 1), binding.RECORD_DTYPE)
    found = C.c_uint64(0)
    if need > 0:                                    # too little room: the error says so, the cursor stays
        before = cur.value
        rc = L.acm_scan_from(handle, C.byref(cur), base + a * sym_bytes, b - a, rec.ctypes.data, need - 1, C.byref(found))
        assert rc == binding.ACM_GPU_E_OVERFLOW and found.value >= need and cur.value == before, (a, b, rc, found.value)
    rc = L.acm_scan_from(handle, C.byref(cur), base + a * sym_bytes, b - a, rec.ctypes.data, need if cap is None else cap, C.byref(found))
    assert rc == 0 and found.value == need, (a, b, rc, found.value, need)
    got = rec[:need].copy()
    got["end_pos"] += np.uint64(a)
    assert np.array_equal(got, want[lo:hi]), (a, b)
    for i in range(b, n):
        assert L.acm_match(C.byref(cur), base + i * sym_bytes) == counts[i], ("tail", a, b, i)
