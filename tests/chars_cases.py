"""Shared by the tests of include/acm_chars.h: the definition in numpy -- cumulative sums of the two byte classes --,
seeded texts (valid UTF-8 mixing characters of 1, 2, 3 and 4 bytes, the same with random bytes written over it, all
ASCII, all continuation bytes), keyword sets like the header's (whole characters, a lone continuation byte, a fragment
that begins inside a character) and the header's worked example."""
import numpy as np

from oracle import pyoracle as po

CODEPOINTS, UTF16 = 1, 2
UNITS = (CODEPOINTS, UTF16)
EDGE_START, EDGE_END, EDGE_BAD = 1, 2, 4
REC = po.RECORD_DTYPE

EXAMPLE_STR = "aé€\U0001F600 é\U0001F600a"
EXAMPLE_TEXT = EXAMPLE_STR.encode("utf-8")
EXAMPLE_KEYWORDS = ["é".encode(), "€\U0001F600".encode(), "\U0001F600".encode(), b"a", b"\xa9", b"\x9f\x98\x80\x20"]
# (end_pos, length, id) -> ((start, len) in code points, (start, len) in UTF-16 units, edge): the header's table
EXAMPLE = [((0, 1, 3), (0, 1), (0, 1), 0), ((2, 2, 0), (1, 1), (1, 1), 0), ((2, 1, 4), (2, 0), (2, 0), 1), ((9, 7, 1), (2, 2), (2, 3), 0),
           ((9, 4, 2), (3, 1), (3, 2), 0), ((10, 4, 5), (4, 1), (5, 1), 1), ((12, 2, 0), (5, 1), (6, 1), 0), ((12, 1, 4), (6, 0), (7, 0), 1),
           ((16, 4, 2), (6, 1), (7, 2), 0), ((17, 1, 3), (7, 1), (9, 1), 0)]
EXAMPLE_TOTALS = (8, 10)

# characters of 1, 2, 3 and 4 bytes the generators draw from
ALPHABET = "ab éß€中\U0001F600\U00010348"
# keyword sets like the example's: whole characters, a lone continuation byte, fragments that begin or end inside a character
KEYWORDS = ["é".encode(), "€\U0001F600".encode(), "\U0001F600".encode(), b"a", b"\xa9", b"\x9f\x98\x80\x20", "b 中".encode(),
            "\U00010348".encode(), b"\x80", b"a\xc3", b"\x9f\x98"]


def as_bytes(text):
    return np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)


def ranks(text):
    """(starts, wides): n + 1 cumulative counts each; count (a, b) is a difference of two entries"""
    t = as_bytes(text)
    starts = np.concatenate(([0], np.cumsum((t & 0xC0) != 0x80))).astype(np.uint64)
    wides = np.concatenate(([0], np.cumsum(t >= 0xF0))).astype(np.uint64)
    return starts, wides


def rank_of(text, unit):
    starts, wides = ranks(text)
    return starts + wides if unit == UTF16 else starts


def text_lo(offsets, n, p):
    """offsets[t] of the text of position(s) p: the largest t with offsets[t] <= p (the last text for p == n)"""
    p = np.asarray(p, dtype=np.uint64)
    if offsets is None or len(offsets) < 2:
        return np.zeros(p.shape, np.uint64), np.full(p.shape, n, np.uint64)
    off = np.asarray(offsets, dtype=np.uint64)
    t = np.minimum(np.searchsorted(off, p, side="right") - 1, off.size - 2)
    return off[t], off[t + 1]


def positions_expected(text, pos, offsets=None, unit=CODEPOINTS):
    t = as_bytes(text)
    r = rank_of(t, unit)
    pos = np.asarray(pos, dtype=np.uint64)
    lo, _ = text_lo(offsets, t.size, pos)
    return r[pos] - r[lo]


def records_expected(text, records, offsets=None, unit=CODEPOINTS, pos_base=0):
    """(char_start u64, char_len u32, edge u8) of every record, by the definition"""
    t = as_bytes(text)
    n = t.size
    r = rank_of(t, unit)
    rec = np.asarray(records, dtype=REC)
    e = rec["end_pos"] - np.uint64(pos_base)
    s = e + np.uint64(1) - rec["length"].astype(np.uint64)
    lo, hi = text_lo(offsets, n, s)
    cont = np.concatenate([(t & 0xC0) == 0x80, [False]])          # (position n: no byte, a boundary)
    e1 = e + np.uint64(1)
    edge = ((s != lo) & cont[s]).astype(np.uint8) | (((e1 != hi) & cont[np.minimum(e1, n)]).astype(np.uint8) << 1)
    return r[s] - r[lo], (r[e1] - r[s]).astype(np.uint32), edge


def valid_text(seed, n_bytes):
    """valid UTF-8 of exactly n_bytes bytes, characters of every width mixed; ASCII fills what is left at the end"""
    rng = np.random.default_rng(seed)
    chars = [c.encode() for c in ALPHABET]
    out, size = [], 0
    while size < n_bytes:
        c = chars[int(rng.integers(0, len(chars)))]
        if size + len(c) > n_bytes:
            c = b"a"
        out.append(c)
        size += len(c)
    text = b"".join(out)
    assert len(text) == n_bytes and text.decode("utf-8") is not None
    return text


def invalid_text(seed, n_bytes, share=0.15):
    """valid_text with random bytes written over a share of it"""
    t = np.frombuffer(valid_text(seed, n_bytes), np.uint8).copy()
    rng = np.random.default_rng(seed + 1000)
    at = rng.integers(0, max(n_bytes, 1), size=int(n_bytes * share))
    if n_bytes:
        t[at] = rng.integers(0, 256, size=at.size, dtype=np.uint8)
    return t.tobytes()


def ascii_text(seed, n_bytes):
    return bytes(np.random.default_rng(seed).integers(32, 127, size=n_bytes, dtype=np.uint8))


def continuation_text(seed, n_bytes):
    return bytes(np.random.default_rng(seed).integers(0x80, 0xC0, size=n_bytes, dtype=np.uint8))


TEXT_KINDS = {"valid": valid_text, "invalid": invalid_text, "ascii": ascii_text, "continuation": continuation_text}


def oracle_of(keywords=KEYWORDS):
    o = po.Oracle(1, po.MEYER85)
    for kw in keywords:
        o.add_keyword(kw)
    return o


def rec_array(triples):
    a = np.zeros(len(triples), REC)
    for i, (e, ln, k) in enumerate(triples):
        a[i] = (e, ln, k)
    return a


def utf16_index(s, i):
    """the index of character i of the str s in UTF-16 code units"""
    return len(s[:i].encode("utf-16-le")) // 2


def find_all(s, keywords):
    """every (start, stop, keyword_id) of the str keywords in the str s, by str.find, in canonical order: by end, then longest first"""
    out = []
    for k, kw in enumerate(keywords):
        at = s.find(kw)
        while at >= 0:
            out.append((at, at + len(kw), k))
            at = s.find(kw, at + 1)
    return sorted(out, key=lambda m: (m[1], -(m[1] - m[0]), m[2]))
