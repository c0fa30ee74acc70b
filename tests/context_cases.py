"""Shared by the context tests (test_context_cpu.py, test_context_gpu.py): the expected answer, which is
always the DEFINITION of CONTEXT (include/acm_gpu.h) in plain Python -- EACH is the window formula,
MERGE a boolean cover array over the buffer: set the windows, cut at the text boundaries under
SYMBOLS, read off the runs -- over the oracle's records or hand-made ones, never the library's own
scan or passes; and a second, independent derivation for TEXTS | MERGE over lines: the groups that
the machine's own `grep -F -C` prints, split at its `--` separators."""
import bisect
import os
import shutil
import subprocess

import numpy as np

from oracle import pyoracle as po

NONE = 0xFFFFFFFF
MOST = 0xFFFFFFFF                     # before = after = 2^32 - 1: everything saturates
KEYWORDS = [b"he", b"she", b"his", b"hers"]


class Expected:
    """n_snippets, snip_lo, lens, out_offsets, snip_text, rec_snip, rec_at as Python lists / numpy arrays"""

    def __init__(self, snip_lo, lens, snip_text, rec_snip, rec_at):
        self.snip_lo = np.array(snip_lo, np.uint64)
        self.lens = np.array(lens, np.uint64)
        self.out_offsets = np.concatenate([[0], np.cumsum(self.lens, dtype=np.uint64)]).astype(np.uint64)
        self.snip_text = np.array(snip_text, np.uint32)
        self.rec_snip = np.array(rec_snip, np.uint32)
        self.rec_at = np.array(rec_at, np.int64)
        self.n_snippets = len(snip_lo)
        self.out_symbols = int(self.out_offsets[-1])

    def out(self, text):
        """the gathered output over `text` (a numpy array of symbols)"""
        t = np.asarray(text)
        parts = [t[int(lo):int(lo) + int(n)] for lo, n in zip(self.snip_lo, self.lens)]
        return np.concatenate(parts) if parts else t[:0]


def _offsets(offsets, n):
    return [0, n] if offsets is None else [int(x) for x in offsets]


def _holder(off, pos):
    """the text with off[t] <= pos < off[t + 1]"""
    t = bisect.bisect_right(off, pos) - 1
    assert 0 <= t < len(off) - 1 and off[t] <= pos < off[t + 1]
    return t


def windows(records, n, offsets=None, before=0, after=0, texts=False, pos_base=0):
    """per record (s, t, lo, hi), lo = hi = None for a windowless record: the window formula"""
    rec = np.asarray(records)
    off = _offsets(offsets, n)
    n_texts = len(off) - 1
    out = []
    for j in range(rec.size):
        e = int(rec["end_pos"][j]) - pos_base
        s = e + 1 - int(rec["length"][j])
        assert 0 <= s <= e < n
        t = _holder(off, s)
        if e >= off[t + 1]:
            out.append((s, t, None, None))
        elif texts:
            out.append((s, t, off[max(0, t - before)], off[min(n_texts, t + 1 + after)]))
        else:
            out.append((s, t, max(off[t], s - before), min(off[t + 1], e + 1 + after)))
    return out


def each(records, n, offsets=None, before=0, after=0, texts=False, pos_base=0):
    """EACH: snippet j is the window of record j; a windowless record gives an empty snippet at its start"""
    off = _offsets(offsets, n)
    w = windows(records, n, offsets, before, after, texts, pos_base)
    lo = [s if a is None else a for s, t, a, b in w]
    lens = [0 if a is None else b - a for s, t, a, b in w]
    at = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    holder = [0 if offsets is None else _holder(off, x) for x in lo]
    return Expected(lo, lens, holder, [NONE if a is None else j for j, (s, t, a, b) in enumerate(w)],
                    [-1 if a is None else int(at[j]) + s - a for j, (s, t, a, b) in enumerate(w)])


def merge(records, n, offsets=None, before=0, after=0, texts=False, pos_base=0):
    """MERGE: the maximal runs of the union of the windows, cut at the text boundaries under SYMBOLS"""
    off = _offsets(offsets, n)
    w = windows(records, n, offsets, before, after, texts, pos_base)
    cover = np.zeros(n + 1, bool)
    for s, t, a, b in w:
        if a is not None:
            cover[a:b] = True
    cut = np.zeros(n + 1, bool)
    if not texts:
        cut[np.array(off, np.int64)] = True
    begins = [p for p in range(n) if cover[p] and (p == 0 or not cover[p - 1] or cut[p])]
    snip_lo, lens = [], []
    for p in begins:
        q = p + 1
        while cover[q] and not cut[q]:
            q += 1
        snip_lo.append(p)
        lens.append(q - p)
    at = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rec_snip, rec_at = [], []
    for s, t, a, b in w:
        if a is None:
            rec_snip.append(NONE)
            rec_at.append(-1)
            continue
        q = bisect.bisect_right(snip_lo, s) - 1                     # the last snippet that begins at or in front of s
        assert snip_lo[q] <= a and b <= snip_lo[q] + lens[q]        # the window lies in one snippet
        rec_snip.append(q)
        rec_at.append(int(at[q]) + s - snip_lo[q])
    return Expected(snip_lo, lens, [0 if offsets is None else _holder(off, p) for p in snip_lo], rec_snip, rec_at)


def expected(records, n, offsets=None, before=0, after=0, texts=False, merged=True, pos_base=0):
    return (merge if merged else each)(records, n, offsets, before, after, texts, pos_base)


def not_vacuous(exp, m):
    """windows were merged, and not all into one"""
    assert 1 < exp.n_snippets < m, (exp.n_snippets, m)
    return exp


def byte_oracle(keywords):
    o = po.Oracle(1, po.MEYER85)
    for kw in keywords:
        o.add_keyword(kw)
    return o


def oracle_records(keywords, text):
    return byte_oracle(keywords).scan(bytes(text)) if len(text) else np.zeros(0, po.RECORD_DTYPE)


BATCH_TEXTS = [b"", b"she sells", b"", b"", b"zz", b"y", b"hers", b"he", b"q", b"", b"ww", b"", b"ushers and his", b"x", b"", b"v", b"uu",
               b"the end: he", b"us", b"hers", b""]


def batch_case():
    """(packed buffer, offsets, the oracle's records of the PACKED buffer): empty texts, a text that is one match, windows
    that touch across a boundary ("hers" | "he"), windows clipped at both ends of their text and records that span a cut"""
    packed = b"".join(BATCH_TEXTS)
    off = np.concatenate([[0], np.cumsum([len(t) for t in BATCH_TEXTS])]).astype(np.uint64)
    return packed, off, oracle_records(KEYWORDS, packed)


def line_offsets(text):
    """the offsets of the lines of `text` (bytes), each with its newline; an unterminated last line counts"""
    cuts = [i + 1 for i, c in enumerate(bytes(text)) if c == 10]
    if len(text) and (not cuts or cuts[-1] != len(text)):
        cuts.append(len(text))
    return np.array([0] + cuts, np.uint64)


def novel_page(novel_bytes, n=4096):
    """(text, records, line offsets) of the novel's first n bytes under {he, she, his, hers}"""
    text = novel_bytes[:n]
    return text, oracle_records(KEYWORDS, text), line_offsets(text)


def have_grep():
    return shutil.which("grep") is not None


def grep_groups(keywords, text, before, after, tmp_path):
    """the context groups `grep -F -B before -A after` prints for `text` (bytes that end with a newline and hold
    no line "--"), as a list of bytes"""
    assert text.endswith(b"\n") and b"\n--\n" not in text and not text.startswith(b"--\n")
    path = os.path.join(str(tmp_path), "page.txt")
    with open(path, "wb") as f:
        f.write(text)
    cmd = ["grep", "-a", "-F", "-B", str(before), "-A", str(after)]
    for kw in keywords:
        cmd += ["-e", kw.decode()]
    p = subprocess.run(cmd + [path], capture_output=True, env=dict(os.environ, LC_ALL="C"))
    assert p.returncode == 0, p.stderr
    groups, cur = [], []
    for line in p.stdout.split(b"\n")[:-1]:
        if line == b"--":
            groups.append(b"".join(cur))
            cur = []
        else:
            cur.append(line + b"\n")
    groups.append(b"".join(cur))
    return groups
