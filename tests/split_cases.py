"""Shared by the split tests (test_split_cpu.py, test_split_gpu.py): the expected offsets, which always
come from numpy on the caller's symbols -- never from the library --, the edge buffers, and the symbols
of 2, 3, 4 and 8 bytes the byte cases are widened to."""
import numpy as np

DELIM1 = b"\n"
DELIM16 = b"\n\t ,;.:!?()[]{}-"
assert len(set(DELIM16)) == 16

# every "\n" below stands for a delimiter (with_delims () deals the members of a larger set out to them)
EDGES = [
    b"",                                   # n = 0
    b"\n",                                 # one symbol that is a delimiter
    b"a",                                  # one that is not
    b"abcxyz",                             # no delimiter at all
    b"\n\n\n\n\n",                         # delimiters only
    b"ab\ncd\n",                           # the last symbol a delimiter
    b"ab\ncd",                             # and not: an unterminated last text
    b"\n\n\nab\n\ncd",                     # a leading run
    b"a\n\nb",                             # the header's example: a\n, \n, b
    b"ab\n\n\n",                           # a run that ends the buffer
]


def with_delims(text, delims):
    """`text` with its newlines replaced by the members of `delims` in turn"""
    out, k = bytearray(text), 0
    for i, c in enumerate(out):
        if c == 10:
            out[i] = delims[k % len(delims)]
            k += 1
    return bytes(out)


def wide(text, sb):
    """bytes -> raw bytes of symbols of sb bytes: the letter c is (c, c ^ 0x5A, 7, 8, ...)[:sb]
    (tests/test_grep_cpu.py::_wide's symbols)"""
    w = np.frombuffer(bytes(text), np.uint8)
    cols = [w, w ^ 0x5A] + [np.full_like(w, 7 + k) for k in range(6)]
    return np.stack(cols[:sb], axis=1).reshape(-1).copy()


def values(raw, sb):
    """raw bytes of symbols of sb bytes -> one uint64 per symbol (its bytes, zero-extended)"""
    r = np.ascontiguousarray(raw).reshape(-1).view(np.uint8).reshape(-1, sb)
    v = np.zeros((r.shape[0], 8), np.uint8)
    v[:, :sb] = r
    return v.reshape(-1).view(np.uint64).copy()


def expected_offsets(sym, delims, runs):
    """the definition in numpy: `sym` one value per symbol, `delims` the delimiter values"""
    sym = np.asarray(sym).reshape(-1)
    if sym.size == 0:
        return np.zeros(1, np.uint64)
    d = np.isin(sym, np.asarray(delims).reshape(-1))
    cut = d & ~np.append(d[1:], False) if runs else d.copy()
    cut[-1] = True
    return np.concatenate([[0], np.flatnonzero(cut) + 1]).astype(np.uint64)


def expected_raw(raw, delims_raw, sb, runs):
    """the same for raw bytes of symbols of sb bytes"""
    return expected_offsets(values(raw, sb), values(delims_raw, sb), runs)


def straddle(sb):
    """(symbols, delimiter) as arrays of the symbol's type: the delimiter is 0x0A in the lowest byte, and
    the first two symbols hold the delimiter's bytes across their boundary.  Only the third symbol is one."""
    dtype = {2: np.uint16, 4: np.uint32, 8: np.uint64}[sb]
    top = np.array([0x0A << (8 * (sb - 1))], np.uint64).astype(dtype)[0]
    text = np.array([top, 0, 0x0A], dtype)
    raw = text.view(np.uint8)
    assert bytes(raw[sb - 1:2 * sb - 1]) == np.array([0x0A], dtype).tobytes()          # the trap is there
    return text, np.array([0x0A], dtype)
