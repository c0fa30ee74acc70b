"""Shared by the whole-word tests (test_words_cpu.py, test_words_gpu.py): the expected answer, which is
always the DEFINITION of WORDS (include/acm_gpu.h) in plain Python over the oracle's / tests/brute.py's
record set -- never the library's own scan or filter --, a second, independent derivation with Python's
`re` for ASCII byte text, and the machine that takes the caller loop on the host with 8-byte symbols."""
import ctypes as C
import re

import numpy as np

import aho_corasick_1975_amd as acm
from oracle import pyoracle as po

LEFT, RIGHT, BOTH = 1, 2, 3
ASCII_WORD = ((0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A))
NOVEL_KEYWORDS = [b"he", b"she", b"his", b"hers", b"the", b"Mrs", b"Dalloway", b"Mrs. Dalloway"]


def is_word(x, ranges):
    return any(lo <= int(x) <= hi for lo, hi in ranges)


def words(records, text, offsets=None, ranges=ASCII_WORD, flags=BOTH, pos_base=0):
    """WORDS by its definition, record by record in the order of the input.  `text` is a sequence of
    symbol values (bytes, or a numpy array of unsigned integers)."""
    rec = np.asarray(records)
    n = len(text)
    off = [0, n] if offsets is None else [int(x) for x in offsets]
    keep = []
    for j in range(rec.size):
        e = int(rec["end_pos"][j]) - pos_base
        s = e + 1 - int(rec["length"][j])
        assert 0 <= s <= e < n
        t = max(k for k in range(len(off) - 1) if off[k] <= s)   # the text with off[t] <= s < off[t + 1]
        assert off[t] <= s < off[t + 1]
        if e >= off[t + 1]:                                      # spans a cut: no match of any text
            continue
        left_ok = s == off[t] or not is_word(text[s - 1], ranges)
        right_ok = e + 1 == off[t + 1] or not is_word(text[e + 1], ranges)
        if (not (flags & LEFT) or left_ok) and (not (flags & RIGHT) or right_ok):
            keep.append(j)
    return rec[np.array(keep, np.int64)].astype(po.RECORD_DTYPE) if keep else np.zeros(0, po.RECORD_DTYPE)


def words_by_re(keywords, text, flags=BOTH):
    """The same for ASCII byte text and the ASCII word set, from the text alone: per keyword the
    overlapping occurrences whose neighbours pass the lookarounds, as a set of (end_pos, length,
    keyword_id)."""
    w = rb"[0-9A-Za-z_]"
    out = set()
    for k, kw in enumerate(keywords):
        left = rb"(?<!" + w + rb")" if flags & LEFT else rb""
        right = rb"(?!" + w + rb")" if flags & RIGHT else rb""
        for m in re.finditer(left + rb"(?=" + re.escape(kw) + right + rb")", bytes(text)):
            out.add((m.start() + len(kw) - 1, len(kw), k))
    return out


def as_set(records):
    return {(int(r["end_pos"]), int(r["length"]), int(r["keyword_id"])) for r in records}


def byte_oracle(keywords):
    o = po.Oracle(1, po.MEYER85)
    for kw in keywords:
        o.add_keyword(kw)
    return o


def oracle_records(keywords, text):
    return byte_oracle(keywords).scan(text) if len(text) else np.zeros(0, po.RECORD_DTYPE)


def novel_case(novel_bytes, n=6000):
    """(keywords, text, raw records, whole-word records) on the novel's opening: the two derivations
    must agree before anything else is compared, and `he` has fewer whole-word than raw matches"""
    text = novel_bytes[:n]
    rec = oracle_records(NOVEL_KEYWORDS, text)
    want = words(rec, text)
    assert as_set(want) == words_by_re(NOVEL_KEYWORDS, text) and len(as_set(want)) == want.size
    for flags in (LEFT, RIGHT):
        assert as_set(words(rec, text, flags=flags)) == words_by_re(NOVEL_KEYWORDS, text, flags)
    raw_he, word_he = int(np.count_nonzero(rec["keyword_id"] == 0)), int(np.count_nonzero(want["keyword_id"] == 0))
    print("records %d, whole-word %d; he: raw %d, whole-word %d" % (rec.size, want.size, raw_he, word_he))
    assert 0 < word_he < raw_he
    return NOVEL_KEYWORDS, text, rec, want


def sym8(word):
    """bytes -> the same word in 8-byte symbols (a numpy uint64 array): the letter c is the integer c"""
    return np.frombuffer(bytes(word), np.uint8).astype(np.uint64)


def loop_machine8(keywords):
    """(handle, keep-alive list) of a machine whose comparator is not ACM_CMP_DEFAULT -- the C library's
    memcmp, called as cmp (a, b, (void *) 8) -- over symbols of 8 bytes, declared with
    acm_set_symbol_bytes: no GPU path takes it (classes are enumerated for 1, 2 and 4 bytes only), its
    calls run the caller loop on the host"""
    L = acm.lib()
    libc = C.CDLL(None)
    h = L.acm_create(C.cast(libc.memcmp, C.c_void_p), C.c_void_p(8), None)
    keep = [libc]
    for kw in keywords:
        buf = sym8(kw).copy()
        keep.append(buf)
        cur = C.c_void_p(L.acm_initiate(h))
        for i in range(len(kw)):
            L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + i * 8)
        L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    assert L.acm_set_symbol_bytes(h, 8) == 0
    return h, keep
