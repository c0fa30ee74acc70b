"""Shared by the tally tests (test_tally_cpu.py, test_tally_gpu.py): the expected answer, which is
always np.bincount over the ORACLE's records -- never the library's own scan --, the check that a
workload cannot pass trivially, the plan kinds of tests/test_batch_gpu.py and the machine that takes
the caller loop on the host."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from oracle import pyoracle as po
from tests.cases import build_pair, build_pair_packed

PATH_GPU, PATH_CLASSES, PATH_LOOP = 1, 2, 3
FORM_LDS, FORM_GLOBAL = 1, 2
ABSENT = b"ABSENT"
PATTERN = np.uint64(0x0123456789ABCDEF)            # what pre-filled counters hold: counter k = PATTERN + k


def oracle_tally(o, text, n_keywords=None, emit_from=0):
    """(bincount of the oracle's records with end_pos >= emit_from, their number)"""
    K = o.nb_keywords if n_keywords is None else n_keywords
    rec = o.scan(text) if len(text) else np.zeros(0, po.RECORD_DTYPE)
    rec = rec[rec["end_pos"] >= emit_from]
    return np.bincount(rec["keyword_id"], minlength=K).astype(np.uint64), int(rec.size)


def nontrivial(want):
    """from the oracle alone: two keywords with different non-zero counts, one keyword without a match"""
    distinct = np.unique(want[want > 0])
    print("keywords %d, with matches %d, distinct non-zero counts %d, matches %d" % (want.size, np.count_nonzero(want), distinct.size,
                                                                                      int(want.sum())))
    assert distinct.size >= 2 and np.any(want == 0), (distinct[:8], int(np.count_nonzero(want == 0)))


def prefilled(n):
    return PATTERN + np.arange(n, dtype=np.uint64)


def kind(name, monkeypatch, kat):
    """(machine, oracle, text, plan maker, check of the plan, expected tally form) of a plan kind:
    tests/test_batch_gpu.py::_kind, the classes case with one keyword more that the novel lacks, the
    delta case with its last keyword replaced by one that the text lacks"""
    n = 1 << 20
    if name == "dense":
        kd, ko = acm.synth.keywords(1000)
        m, o = build_pair_packed(kd, ko)
        return m, o, acm.synth.text(n, kd, ko), m.plan, lambda p: p.info.kernel == 1, FORM_LDS
    if name == "gram":
        kd, ko = acm.synth.keywords(20000)
        m, o = build_pair_packed(kd, ko, variant=po.MEYER85)
        return m, o, acm.synth.text(n, kd, ko), m.plan, lambda p: p.info.kernel == 5, FORM_GLOBAL
    if name == "csr":
        # the CSR walk is what a DENSE plan (no class table) launches on a text that is not 16-byte aligned
        kd, ko = acm.synth.keywords(1000)
        m, o = build_pair_packed(kd, ko)
        return m, o, acm.synth.text(n, kd, ko), m.plan, lambda p: p.info.kernel == 1 and p.info.records_direct == 0, FORM_LDS
    if name in ("starts", "walk"):
        if name == "walk":
            monkeypatch.setenv("ACM_GPU_SPARSE", "walk")
        kd, ko = acm.synth.keywords(2000, sym_bytes=4, vocab=500)
        m, o = build_pair_packed(kd, ko, sym_size=4)
        return (m, o, acm.synth.text(n, kd, ko, sym_bytes=4, vocab=500), m.plan, lambda p: p.info.kernel == (3 if name == "walk" else 4),
                FORM_LDS)
    if name == "u64":
        rng = np.random.default_rng(8)
        vocab = rng.integers(0, 1 << 63, size=3000, dtype=np.uint64)
        kws = [vocab[rng.integers(0, vocab.size, size=rng.integers(1, 7))] for _ in range(1500)]
        m, o = build_pair(kws, 8)
        text = vocab[rng.integers(0, vocab.size, size=200003)]
        noise = rng.integers(0, text.size, size=20000)
        text[noise] = rng.integers(0, 1 << 63, size=noise.size, dtype=np.uint64)
        for _ in range(3000):
            w = kws[int(rng.integers(0, len(kws)))]
            at = int(rng.integers(0, text.size - w.size))
            text[at:at + w.size] = w
        return m, o, text, m.plan, lambda p: p.info.kernel == 4, FORM_LDS
    if name == "classes":
        cmp = C.cast(kat.kat_casecmp8, C.c_void_p)
        m = acm.Machine(1, cmp=cmp)
        o = po.Oracle(1, po.MEYER85, cmp=cmp)
        for kw in (b"He", b"SHE", b"his", b"hErs", b"Mrs", b"dalloway", b"Zyzzyva"):
            m.add_keyword(kw)
            o.add_keyword(kw)
        m.set_symbol_bytes(1)
        return m, o, None, m.plan_classes, lambda p: p.info.kernel == 1, FORM_LDS
    assert name == "delta"
    # (every one of the 450 synthetic keywords occurs in the text: the 450th is replaced by one that cannot)
    kd, ko = acm.synth.keywords(450)
    m, o = build_pair_packed(kd[:ko[300]], ko[:301], variant=po.MEYER85)

    def plan_then_update(device):
        plan = m.plan(device)
        for k in range(300, 449):
            m.add_keyword(kd[ko[k]:ko[k + 1]])
            o.add_keyword(kd[ko[k]:ko[k + 1]])
        m.add_keyword(ABSENT)                          # the delta's last keyword: one the text (a-z) cannot hold
        o.add_keyword(ABSENT)
        plan.update(m)
        return plan
    return m, o, acm.synth.text(n, kd, ko), plan_then_update, lambda p: p.info.delta_keywords == 150 and p.info.merges == 0, FORM_LDS


KINDS = ["dense", "gram", "csr", "starts", "walk", "u64", "classes", "delta"]


def planted(text, seed):
    """`text` with 500 copies of six keywords of the 4-gram kind's dictionary (4 symbols or more each) written over it at
    random: its own text holds a planted keyword per 4,096 symbols, too few for a selection or a pattern to tell"""
    kd, ko = acm.synth.keywords(20000)
    six = [k for k in range(ko.size - 1) if ko[k + 1] - ko[k] >= 4][:6]
    rng = np.random.default_rng(seed)
    t = text.copy()
    for k in rng.choice(six, size=500):
        w = kd[ko[k]:ko[k + 1]]
        at = int(rng.integers(0, t.size - w.size))
        t[at:at + w.size] = w
    return t


# ---- the machine without a GPU path: a comparator of its own over 3-byte symbols
def sym3(word):
    """bytes -> the same word in 3-byte symbols (as bytes): the letter c is (c, c ^ 0x5A, 7) for the
    machine and the byte c for the oracle -- one to one, so both see the same equal and unequal symbols"""
    w = np.frombuffer(bytes(word), np.uint8)
    return np.stack([w, w ^ 0x5A, np.full_like(w, 7)], axis=1).tobytes()


def loop_machine(keywords):
    """(handle, keep-alive list) of a machine whose comparator is not ACM_CMP_DEFAULT -- the C library's
    memcmp, called as cmp (a, b, (void *) 3) -- over symbols of 3 bytes, declared with
    acm_set_symbol_bytes: no GPU path takes it, acm_tally runs the caller loop on the host"""
    L = acm.lib()
    libc = C.CDLL(None)
    h = L.acm_create(C.cast(libc.memcmp, C.c_void_p), C.c_void_p(3), None)
    keep = [libc]
    for kw in keywords:
        buf = np.frombuffer(sym3(kw), dtype=np.uint8).copy()
        keep.append(buf)
        cur = C.c_void_p(L.acm_initiate(h))
        for i in range(len(kw)):
            L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + i * 3)
        L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    assert L.acm_set_symbol_bytes(h, 3) == 0
    return h, keep


def byte_oracle(keywords):
    o = po.Oracle(1, po.MEYER85)
    for kw in keywords:
        o.add_keyword(kw)
    return o


def novel_words(novel_bytes, n=400):
    """a dictionary of the novel's own words: its n most frequent distinct words of 3 letters or more
    in order of first appearance, and two words it does not hold"""
    import re
    words = re.findall(rb"[A-Za-z]{3,}", novel_bytes)
    seen = {}
    for w in words:
        seen[w] = seen.get(w, 0) + 1
    top = set(sorted(seen, key=lambda w: (-seen[w], w))[:n])
    first = []
    for w in words:
        if w in top:
            top.discard(w)
            first.append(w)
    return first + [b"zyzzyva", b"qwertyuiop"]
