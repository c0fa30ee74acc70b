"""Dictionaries and texts with LONG keywords (64 to 9,000 symbols), shared by test_long_keywords_cpu.py
and test_long_keywords_gpu.py so that a GPU failure can be bisected to the input, to the flattener or
to the kernel.  lmax (the longest keyword) decides the plan kind (4081 is the last dense plan, 4082 a
CSR plan), the halo of shards, segments and stream pieces, the order passes (tiled up to 1024), the
form of SELECT (tiled up to 1024) and the width of the length field of sort keys and wire words
(a bit more at 64, 128, 256, ...): CASES stands on both sides of each of those."""
import numpy as np

import aho_corasick_1975_amd as acm
from oracle import pyoracle as po

DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}
BOUNDARIES = (64, 1024, 8192, 65536)   # dense chunk, 4-gram group, tile, test-sized launch segment
RUN_EXTRA = 256                        # the periodic run is lmax + RUN_EXTRA symbols long


def boundary_sizes(lmax):
    """BOUNDARIES, largest first (the fewest multiples), and the CSR walk's chunk per lane of a short text"""
    return BOUNDARIES[::-1] + ((8 * lmax,) if 8 * lmax not in BOUNDARIES else ())


def fixed_regions(n, lmax):
    """[begin, end) of what long_case writes last: first and last possible match, near miss, periodic run"""
    return [(0, lmax), (n - lmax, n), (n // 2, n // 2 + lmax), (n // 3, n // 3 + lmax + RUN_EXTRA)]


def long_case(seed, sym, lmax, n_long, n, lo, span, shorts=True, filler=0):
    """(keywords, text).  keywords[0] is the spine S (lmax random symbols), keywords[1] the periodic
    P = abab... (lmax symbols: self-overlapping, deep failure links); n_long - 2 more long keywords;
    suffixes of S (several long records at ONE end position), prefixes of S (outputs on the way down
    a long match), an infix, and keywords of 1-4 symbols (shorts=False: nothing below 4 symbols);
    `filler` random keywords of 4-12 symbols.  The text is random over the alphabet and one symbol
    on either side of it; S is planted across multiples of every size in boundary_sizes (lmax) -- at
    random offsets and at the two extremes, one symbol behind and one symbol before the multiple --, at
    the very start and the very end; at n/2 stands S with its last symbol wrong; at n/3 a run of abab... in
    which P ends at every second position."""
    assert lo >= 1 and span >= 2 and lmax >= 16 and n >= 8 * lmax
    rng = np.random.default_rng(seed)
    dt = DTYPES[sym]

    def A(k):
        return rng.integers(lo, lo + span, size=int(k)).astype(dt)

    S = A(lmax)
    P = np.resize(np.array([lo, lo + 1], dt), lmax)
    kws = [S, P] + [A(rng.integers(lmax // 2, lmax + 1)) for _ in range(n_long - 2)]
    kws += [S[k:] for k in (1, lmax // 3, lmax - 5, lmax - 1)]
    kws += [S[:k] for k in (2, 5, lmax // 2, lmax - 1)]
    kws += [S[lmax // 4:lmax // 4 + 7]] + ([A(1), A(2), A(3), A(4)] if shorts else [A(4)])
    kws += [A(rng.integers(4, 13)) for _ in range(filler)]
    if not shorts:
        kws = [w for w in kws if w.size >= 4]
    text = rng.integers(lo - 1, lo + span + 1, size=n).astype(dt)
    fixed = fixed_regions(n, lmax)
    per_size = int(max(2, min(40, n // (8 * lmax))))    # plants of one size: at most an eighth of the text
    for b in BOUNDARIES:
        free = [m for m in range(b, n, b) if all(m + lmax <= f0 or m - lmax >= f1 for f0, f1 in fixed)]
        for m in free[::max(1, len(free) // per_size)][:per_size]:
            start = m - int(rng.integers(1, lmax))      # 1 .. lmax-1 symbols before the multiple: S crosses it
            text[start:start + lmax] = S
    # the two extremes at every size, written after the random plants and clear of one another: all of
    # S but its last symbol before a multiple (whoever starts reading at the multiple needs every
    # symbol of an lmax-1 halo), and all of S but its first symbol behind one
    taken = list(fixed)
    for b in boundary_sizes(lmax):
        for back in (lmax - 1, 1):
            for m in range(b, n, b):
                if all(m - back + lmax <= t0 or m - back >= t1 for t0, t1 in taken):
                    text[m - back:m - back + lmax] = S
                    taken.append((m - back, m - back + lmax))
                    break
    text[:lmax] = S
    text[n - lmax:] = S
    text[n // 2:n // 2 + lmax - 1] = S[:-1]
    text[n // 2 + lmax - 1] = lo - 1
    text[n // 3:n // 3 + lmax + RUN_EXTRA] = np.resize(P[:2], lmax + RUN_EXTRA)
    return kws, text


N18, N20 = 1 << 18, 1 << 20

# name -> (long_case arguments, environment switches, what ACMPlanInfo must say).  In `expect`,
# "variant_set" / "variant_clear" are bits of ACMPlanInfo::variant; "sticky" asks for more than
# 32,768 dense rows (4-byte entries).  Both sides of a threshold are cases of their own.
CASES = {}


def _case(name, env, expect, **kw):
    CASES[name] = (dict(seed=9000 + len(CASES), **kw), env, expect)


for _l in (64, 65, 255, 256, 1024, 1025, 2049, 4081):      # continuation mode (2-byte entries); 255/256: a length bit more
    _case("dense-%d" % _l, {}, dict(kernel=1, entry_bytes=2), sym=1, lmax=_l, n_long=4, n=N18, lo=97, span=4)
for _l in (256, 4081):                                      # sticky mode: more than 32,768 states
    _case("sticky-%d" % _l, {"ACM_GPU_GRAM": "0"}, dict(kernel=1, entry_bytes=4, sticky=True),
          sym=1, lmax=_l, n_long=14, n=N18, lo=97, span=26, filler=6000)
for _l in (4082, 5000, 9000):                               # lmax - 1 > 16 * 255: no dense rows, the CSR walk
    _case("csr-%d" % _l, {}, dict(kernel=2, entry_bytes=0, records_direct=1), sym=1, lmax=_l, n_long=4, n=N18, lo=97, span=4)
for _l in (64, 1024, 1025, 4081):                           # scan_gram2_kernel; one-pass tiled order up to 1024
    _case("gram2-%d" % _l, {"ACM_GPU_GRAM": "2"}, dict(kernel=5, variant_set=2, variant_clear=4, records_direct=1),
          sym=1, lmax=_l, n_long=4, n=N18, lo=97, span=8, shorts=False, filler=300)
_case("gram2short-1025", {"ACM_GPU_GRAM": "2"}, dict(kernel=5, variant_set=2 | 4, records_direct=1),
      sym=1, lmax=1025, n_long=4, n=N18, lo=97, span=8, filler=300)
for _l in (1024, 1025):                                     # scan_gram_kernel
    _case("gramold-%d" % _l, {"ACM_GPU_GRAM": "2", "ACM_GPU_GRAM2": "0"}, dict(kernel=5, variant_clear=2 | 4, records_direct=1),
          sym=1, lmax=_l, n_long=4, n=N18, lo=97, span=8, shorts=False, filler=300)
for _l in (256, 1025):                                      # hashed 4-byte windows: more than 29 symbols in use
    _case("hashed-%d" % _l, {"ACM_GPU_GRAM": "3"}, dict(kernel=5, records_direct=0), sym=1, lmax=_l, n_long=4, n=N18, lo=60, span=40)
for _s in (2, 4):
    for _l in (65, 1025, 5000):                             # start-parallel kernel: a keyword longer than a group and a tile
        _case("starts%d-%d" % (8 * _s, _l), {}, dict(kernel=4), sym=_s, lmax=_l, n_long=4, n=N18, lo=1000, span=300)
    for _l in (65, 1025):
        _case("walk%d-%d" % (8 * _s, _l), {"ACM_GPU_SPARSE": "walk"}, dict(kernel=3), sym=_s, lmax=_l, n_long=4, n=N18, lo=1000, span=300)
# 2^20 symbols: sixteen launch segments of 2^16 symbols
_case("dense-1025-seams", {}, dict(kernel=1, entry_bytes=2), sym=1, lmax=1025, n_long=4, n=N20, lo=97, span=4)
_case("gram2-1025-seams", {"ACM_GPU_GRAM": "2"}, dict(kernel=5, variant_set=2, variant_clear=4, records_direct=1),
      sym=1, lmax=1025, n_long=4, n=N20, lo=97, span=8, shorts=False, filler=300)

# 2^15 symbols: a stream fed seven symbols at a time makes a launch per piece
_case("dense-65-short", {}, dict(kernel=1, entry_bytes=2), sym=1, lmax=65, n_long=4, n=1 << 15, lo=97, span=4)

# (case, log2 of the launch segment).  2^12-symbol segments: a halo of lmax - 1 = 4,999 symbols is
# longer than the segment and a keyword crosses two seams; the families with dense rows stop at
# lmax = 4081 (a halo of 4,080 symbols: a keyword crosses one seam and reaches the next).
SEAM_CASES = [("dense-4081", 12), ("gram2-4081", 12), ("starts32-5000", 12), ("csr-5000", 12),
              ("dense-1025-seams", 16), ("gram2-1025-seams", 16), ("starts32-1025", 16), ("csr-4082", 16)]


def seams_crossed(name, seg_log2):
    """how many segment seams each full-length match of S lies across"""
    ends = spine_ends(name)
    return (ends >> seg_log2) - ((ends - CASES[name][0]["lmax"] + 1) >> seg_log2)


_built = {}
_answers = {}


def params(name):
    return CASES[name][0]


def case(name):
    """(keywords, text) of a case, made once"""
    if name not in _built:
        _built[name] = long_case(**CASES[name][0])
        _built[name][1].setflags(write=False)
    return _built[name]


def answer(name):
    """(oracle machine, its records of the whole text), made once and left unchanged"""
    if name not in _answers:
        kws, text = case(name)
        o = po.Oracle(CASES[name][0]["sym"], po.AC75)
        for w in kws:
            o.add_keyword(w)
        want = o.scan(text)
        want.setflags(write=False)
        _answers[name] = (o, want)
    return _answers[name]


def machine(name):
    """a product machine with the case's keywords (a new one each time: plans and updates belong to the test)"""
    m = acm.Machine(CASES[name][0]["sym"])
    for w in case(name)[0]:
        m.add_keyword(w)
    return m


def assert_family(name, info):
    """the plan is of the kernel family the case is meant for"""
    e = CASES[name][2]
    got = {f: getattr(info, f) for f in ("kernel", "entry_bytes", "variant", "records_direct", "dense_rows")}
    for f in ("kernel", "entry_bytes", "records_direct"):
        if f in e:
            assert got[f] == e[f], (name, f, got)
    assert got["variant"] & e.get("variant_set", 0) == e.get("variant_set", 0), (name, got)
    assert got["variant"] & e.get("variant_clear", 0) == 0, (name, got)
    if e.get("sticky"):
        assert got["dense_rows"] > 32768, (name, got)


def spine_ends(name):
    """end positions of the full-length matches of S (keyword 0), from the oracle"""
    _, want = answer(name)
    lmax = CASES[name][0]["lmax"]
    return want["end_pos"][(want["keyword_id"] == 0) & (want["length"] == lmax)].astype(np.int64)
