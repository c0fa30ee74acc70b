"""Record positions across the 2^32 carry and with bit 63 set, on the GPU.  The kernels move the
64-bit pos_base and end_pos as two 32-bit words; here every text is placed so that a planted
occurrence lies across position 2^32 (WRAP32) or 2^63 + 2^32 (TOP), and the canonical order is run on
positions and lengths that the radix sort's old single key could not hold.  The expected answer is
always the family's Python definition over the ORACLE's records at pos_base = 0, then translated
(tests/position_cases.py); everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from oracle import pyoracle as po
from tests import long_cases
from tests import position_cases as pcase
from tests.cases import build_pair
from tests.position_cases import NAMES, bases, boundary_inside, breach_positions, canonical, extent, moved, straddles, thirds
from tests.tally_cases import KINDS

pytestmark = pytest.mark.gpu

N_SCAN = 1 << 16


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _dev(torch, arr):
    a = np.frombuffer(bytes(arr), dtype=np.uint8) if isinstance(arr, (bytes, bytearray)) else np.ascontiguousarray(arr)
    a = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])
    return torch.from_numpy(a.copy()).cuda()


def _rec_dev(torch, rec, room=None):
    a = np.zeros(max(rec.size if room is None else room, 1), po.RECORD_DTYPE)
    a[:rec.size] = rec
    return torch.from_numpy(a.view(np.int64).reshape(-1, 2).copy()).cuda()


def _rec_host(t, n):
    return np.frombuffer(t[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()


def _same(got, want, what=None):
    got = np.asarray(got).astype(po.RECORD_DTYPE)
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first difference at record %d of %d" % (bad[0], want.size), got[bad[:4]], want[bad[:4]])


# ---------------------------------------------------------------- a. the core scan
def _scan_checks(torch, monkeypatch, plan, dev, n, text_host, all_rec, c, what):
    """every way to the records of one text, at both bases, whole and from a cut three symbols in front
    of the boundary"""
    for name in NAMES:
        base = bases(c)[name]
        for emit_from in (0, c - 3):
            want = moved(all_rec[all_rec["end_pos"] >= emit_from], base)
            tag = (what, name, emit_from)
            cap = want.size + 8
            rec, cnt = plan.scan(dev, emit_from=emit_from, pos_base=base, capacity=cap)
            assert int(cnt.item()) == want.size, tag
            _same(canonical(_rec_host(rec, want.size)), want, tag + ("scan",))
            _same(plan.scan_sorted(dev, emit_from=emit_from, pos_base=base, capacity=cap), want, tag + ("scan_ordered",))
            _same(plan.scan_sorted(dev, emit_from=emit_from, pos_base=base, capacity=cap, fused=False), want, tag + ("scan, order",))
            monkeypatch.setenv("ACM_GPU_ORDER", "radix")
            _same(plan.scan_sorted(dev, emit_from=emit_from, pos_base=base, capacity=cap, fused=False), want, tag + ("scan, radix order",))
            _same(plan.scan_sorted(dev, emit_from=emit_from, pos_base=base, capacity=cap), want, tag + ("scan_ordered, radix",))
            monkeypatch.delenv("ACM_GPU_ORDER")
            if text_host is not None:
                _same(plan.scan_host(text_host, emit_from=emit_from, pos_base=base), want, tag + ("scan_host",))
            # on the wire: pack with pos_lo = base and the widths of a span of n positions, and back
            d_want = _rec_dev(torch, want)
            pb, lb, kb = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            assert acm.lib().acm_gpu_wire_bits(plan.h, n, C.byref(pb), C.byref(lb), C.byref(kb)) == 0, tag
            assert pb.value + lb.value + kb.value <= 64 and (1 << pb.value) >= n
            packed = torch.empty(want.size, dtype=torch.int64, device="cuda")
            back = torch.full((want.size, 2), -1, dtype=torch.int64, device="cuda")
            L = acm.lib()
            assert L.acm_gpu_pack_records_device(d_want.data_ptr(), want.size, base, pb.value, lb.value, packed.data_ptr(), None) == 0
            assert L.acm_gpu_unpack_records_device(packed.data_ptr(), want.size, base, pb.value, lb.value, back.data_ptr(), None) == 0
            torch.cuda.synchronize()
            words = packed.cpu().numpy().view(np.uint64)
            assert np.array_equal(words & np.uint64((1 << pb.value) - 1), all_rec["end_pos"][all_rec["end_pos"] >= emit_from]), tag + ("packed",)
            _same(_rec_host(back, want.size), want, tag + ("unpacked",))
    plan.status()


@pytest.mark.parametrize("name", KINDS)
def test_core_scan_of_every_plan_kind(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """64 Ki symbols of the kind's text (eight 8,192-symbol tiles, sixteen 4,096-position buckets), the
    carry inside a planted keyword near the middle"""
    m, o, text, c, rec, plan = pcase.scan_case(name, monkeypatch, kat, novel_bytes, device=0)
    if name == "csr":
        dev = _dev(torch_cuda, np.concatenate([text[:1], text]))[1:]                 # 1 byte past a 16-byte boundary
        assert dev.data_ptr() % 16 == 1 and dev.is_contiguous()
    else:
        dev = _dev(torch_cuda, text)
    # (acm_gpu_scan_host copies the text to a buffer of its own: the misaligned case has no host form)
    _scan_checks(torch_cuda, monkeypatch, plan, dev, len(text), None if name == "csr" else text, rec, c, name)


def test_core_scan_gram_text_full_of_matches(torch_cuda, monkeypatch):
    """the tiled one-pass order (dev_tiles.h) with nine records at every position: a^4 .. a^12 over 64 Ki
    a's, so that the carry falls inside a crowded bucket of the tile it is in"""
    monkeypatch.setenv("ACM_GPU_GRAM", "2")
    kws = [b"a" * k for k in range(4, 13)] + [b"abab", b"baba", b"aabb"]
    m, o = build_pair(kws, 1)
    plan = m.plan(0)
    assert plan.info.kernel == 5 and plan.info.records_direct == 1, plan.describe()
    text = np.full(N_SCAN, ord("a"), dtype=np.uint8)
    rec = o.scan(text)
    c = N_SCAN // 2 + 1000                                                           # (not on a bucket's or a tile's edge)
    straddles(rec, c)
    assert rec.size == 9 * N_SCAN - sum(range(3, 12))
    _scan_checks(torch_cuda, monkeypatch, plan, _dev(torch_cuda, text), text.size, text, rec, c, "gram, full")


# ---------------------------------------------------------------- b. the canonical order
def _sorted_on_device(torch, plan, rec, pos_lo=None, span=None):
    dev = _rec_dev(torch, rec)
    plan.sort(dev, rec.size, pos_lo, span)
    torch.cuda.synchronize()
    plan.status()
    return _rec_host(dev, rec.size)


def _byte_plan_lmax_12():
    m, o = build_pair([b"a" * k for k in range(1, 13)] + [b"ab", b"ba", b"bab"], 1)
    rng = np.random.default_rng(1975)
    text = rng.choice(np.frombuffer(b"aaab", np.uint8), size=1200)
    return m, o.scan(text)


def _long_plan_lmax_9000():
    name = "csr-9000"
    _, want = long_cases.answer(name)
    ends = long_cases.spine_ends(name)
    mid = int(ends[ends.size // 2])                                                 # a full-length match of S: 9,000 symbols across c
    near = want[(want["end_pos"] > mid - 30000) & (want["end_pos"] < mid + 30000)]
    return long_cases.machine(name), near


@pytest.mark.parametrize("which", ["lmax12", "lmax9000"])
def test_sort_records_across_the_last_position_a_shifted_key_holds(torch_cuda, monkeypatch, which):
    """acm_gpu_sort_records_device on oracle records moved so that position 2^(64 - len_bits) lies inside
    one of them: len_bits = 4 (a byte plan, lmax 12) and 14 (lmax 9,000).  True 64-bit order wanted."""
    if which == "lmax9000":
        for k, v in long_cases.CASES["csr-9000"][1].items():
            monkeypatch.setenv(k, v)
    m, rec = _byte_plan_lmax_12() if which == "lmax12" else _long_plan_lmax_9000()
    len_bits = 4 if which == "lmax12" else 14
    assert (1 << (len_bits - 1)) <= m.lmax < (1 << len_bits)
    rec = rec[:6000]
    assert 3000 <= rec.size <= 6000, rec.size
    lo = int(rec["end_pos"].min())
    rec = moved(rec, -lo)
    c = boundary_inside(rec, int(rec["end_pos"].max()) // 2)
    straddles(rec, c)
    plan = m.plan(0)
    for name, base in bases(c, len_bits).items():
        want = moved(rec, base)
        assert np.array_equal(canonical(want), want), name                          # (translation keeps the order: nothing wraps past 2^64)
        shuffled = want[np.random.default_rng(len_bits).permutation(want.size)]
        _same(_sorted_on_device(torch_cuda, plan, shuffled), want, (which, name))
    edge = 1 << (64 - len_bits)
    want = moved(rec, bases(c, len_bits)["SORT_EDGE"])
    assert int(want["end_pos"].min()) < edge <= int(want["end_pos"].max())


@pytest.mark.parametrize("which", ["lmax12", "lmax9000"])
def test_sort_records_longer_than_the_plans_longest_keyword(torch_cuda, monkeypatch, which):
    """what chains, patterns, approx and edit emit: lengths above the plan's lmax.  At equal end_pos the
    longer record comes first, whatever its length: 64, 2^20, 2^31 and 2^32 - 1 beside 1 .. 12"""
    if which == "lmax9000":
        for k, v in long_cases.CASES["csr-9000"][1].items():
            monkeypatch.setenv(k, v)
    m = _byte_plan_lmax_12()[0] if which == "lmax12" else long_cases.machine("csr-9000")
    plan = m.plan(0)
    lengths = np.array([1, 2, 3, 12, 15, 16, 17, 64, 9000, 16383, 16384, 1 << 20, (1 << 20) + 1, 1 << 31, (1 << 31) + 5, (1 << 32) - 1], np.uint64)
    positions = np.array([5, 6, (1 << 32) - 1, 1 << 32, (1 << 63) + 9, (1 << 64) - 1], np.uint64)
    rec = np.zeros(lengths.size * positions.size, po.RECORD_DTYPE)
    rec["end_pos"] = np.repeat(positions, lengths.size)
    rec["length"] = np.tile(lengths, positions.size)
    rec["keyword_id"] = np.arange(rec.size)
    want = canonical(rec)
    assert np.all(want["length"][:lengths.size] == lengths[::-1].astype(np.uint32)) and want["end_pos"][0] == 5
    for seed in (1, 2):
        _same(_sorted_on_device(torch_cuda, plan, rec[np.random.default_rng(seed).permutation(rec.size)]), want, (which, seed))


def test_order_records_over_a_span_of_2_to_the_62(torch_cuda):
    """acm_gpu_order_records_device with a range the buckets cannot take: 600 records spread over
    span = 2^62 from pos_lo = 2^61 + 7 (bits(span) + len_bits > 64), two at the very ends of the range"""
    m, _ = _byte_plan_lmax_12()
    plan = m.plan(0)
    rng = np.random.default_rng(62)
    pos_lo, span = (1 << 61) + 7, 1 << 62
    off = np.unique(np.concatenate([rng.integers(0, span, size=500, dtype=np.uint64), np.array([0, span - 1, (1 << 60) - 1, 1 << 60], np.uint64)]))
    off = np.concatenate([off, off[:90]])                                           # 90 positions twice: the length decides
    rec = np.zeros(off.size, po.RECORD_DTYPE)
    rec["end_pos"] = off + np.uint64(pos_lo)
    rec["length"] = np.concatenate([rng.integers(1, 7, size=off.size - 90), rng.integers(7, 13, size=90)])
    rec["keyword_id"] = rng.integers(0, 1 << 30, size=off.size)
    rec = rec[rng.permutation(rec.size)]
    want = canonical(rec)
    assert int(want["end_pos"][0]) == pos_lo and int(want["end_pos"][-1]) == pos_lo + span - 1 >= 1 << 62
    _same(_sorted_on_device(torch_cuda, plan, rec, pos_lo, span), want)


# ---------------------------------------------------------------- c. the families
E_INTERNAL = -7
DROPS = ("select", "segment", "words", "patterns", "chains", "approx", "edit", "templates")   # a stranger is dropped, the rest is answered
_machines = {}


def _machine(family, sb):
    """(machine, plan) holding the family's keywords in the order of their ids: a dense plan for bytes, the
    start-parallel kernel for 4-byte symbols; made once per (dictionary, symbol size)"""
    if family == "patterns":
        key, kws = ("patterns", 1), [bytes(k) for k in pcase.pattern_case()[0]]
    elif family == "chains":
        key, kws = ("chains", 1), list(pcase.chain_case()[0])
    elif family in ("approx", "edit"):
        key, kws = ("approx", sb), [np.array(k, pcase.SYM[sb]) for k in pcase.approx_case(sb)[2][0]]
    elif family == "templates":
        key, kws = ("templates", sb), [np.array(k, pcase.SYM[sb]) for k in pcase.template_case(sb)[2][0]]
    else:
        key, kws = ("words", sb), pcase.word_case(sb)[0]
    if key not in _machines:
        m = acm.Machine(sb)
        for kw in kws:
            m.add_keyword(kw)
        plan = m.plan(0)
        assert plan.info.kernel == (1 if sb == 1 else 4) and plan.sym_size == sb, plan.describe()
        _machines[key] = (m, plan)
    return _machines[key]


def _np(t, n, dtype):
    return t[:n].cpu().numpy().view(dtype).copy()


def _snippets(s):
    k, m = s.n_snippets, s.count
    if hasattr(s.snip_lo, "cpu"):
        out = s.out[:s.out_symbols * s.sym_size].cpu().numpy().view(pcase.SYM[s.sym_size])
        return (_np(s.snip_lo, k, np.uint64), _np(s.out_offsets, k + 1, np.uint64), _np(s.snip_text, k, np.uint32), _np(s.rec_snip, m, np.uint32),
                _np(s.rec_at, m, np.int64), out)
    return s.snip_lo, s.out_offsets, s.snip_text, s.rec_snip, s.rec_at, s.out


def _tokens(t, batch):
    k = t.n_tokens
    assert k <= t.token_capacity
    return (_np(t.ids, k, np.uint32), _np(t.length, k, np.uint32)) + ((t.first.cpu().numpy().view(np.uint64),) if batch else ()), _np(t.start, k, np.uint64)


def _replaced(r, sb, n_sel):
    assert r.out_symbols <= r.out_capacity and r.count == n_sel
    return r.out[:r.out_symbols * sb].cpu().numpy().view(pcase.SYM[sb]).copy(), _np(r.out_start, n_sel, np.uint64)


def _sets(family, sb, plan):
    tset, nk = pcase.sets_of(family, sb)
    return tset


def _join(torch, family, sb, plan, records, base, offsets=None):
    """the family's *_records_device call on `records` (host, positions base + index): (records or None, rest, tok_start or None)"""
    text = pcase.inputs(family, sb)[0]
    n, dev, d_rec = text.size, _dev(torch, text), _rec_dev(torch, records)
    d_off = _dev(torch, offsets.astype(np.int64)) if offsets is not None else None
    tset = _sets(family, sb, plan)
    if family == "select":
        out, k = plan.select_records(d_rec, records.size, base, n)
        return _rec_host(out, k), (), None
    if family == "segment":
        out, k, sums = plan.segment_records(d_rec, records.size, base, n, _dev(torch, np.array(pcase.SEGMENT_COST, np.uint32)), pcase.SEGMENT_GAP)
        return _rec_host(out, k), (np.array(sums, np.uint64),), None
    if family == "words":
        out, cnt = plan.words_records(dev, d_rec, records.size, offsets=d_off, ranges=pcase.ranges_of(sb), pos_base=base)
        return _rec_host(out, int(cnt.item())), (), None
    if family == "context":
        return None, _snippets(plan.context_records(dev, d_rec, records.size, offsets=d_off, before=pcase.CONTEXT_BEFORE, after=pcase.CONTEXT_AFTER, pos_base=base)), None
    if family == "replace":
        assert offsets is None
        return None, _replaced(plan.replace_records(dev, d_rec, records.size, pcase.replacements_of(sb), pos_base=base, out_start=True), sb, records.size), None
    if family == "tokens":
        rest, start = _tokens(plan.tokens_records(dev, d_rec, records.size, offsets=d_off, mode="run", gap_base=pcase.TOKEN_GAP_BASE, pos_base=base), offsets is not None)
        return None, rest, start
    if family in ("patterns", "chains"):
        out, cnt = (plan.patterns_records if family == "patterns" else plan.chains_records)(d_rec, records.size, tset, n, offsets=d_off, pos_base=base)
        return _rec_host(out, int(cnt.item())), (), None
    fn = {"approx": plan.approx_records, "edit": plan.edit_records, "templates": plan.templates_records}[family]
    out, dist, cnt = fn(d_rec, records.size, tset, dev, offsets=d_off, pos_base=base)
    k = int(cnt.item())
    return _rec_host(out, k), (_np(dist, k, np.uint32),), None


def _fused(torch, family, sb, plan, base):
    """the family's scan_* device call on the text at pos_base = base"""
    text, rec = pcase.inputs(family, sb)
    dev, cap = _dev(torch, text), rec.size + 8
    tset = _sets(family, sb, plan)
    if family == "select":
        out, cnt, _ = plan.scan_select(dev, pos_base=base, capacity=cap)
        return _rec_host(out, int(cnt.item())), (), None
    if family == "segment":
        out, cnt, sums, _ = plan.scan_segment(dev, _dev(torch, np.array(pcase.SEGMENT_COST, np.uint32)), pcase.SEGMENT_GAP, pos_base=base, capacity=cap)
        return _rec_host(out, int(cnt.item())), (sums.cpu().numpy().view(np.uint64),), None
    if family == "words":
        out, cnt, _ = plan.scan_words(dev, ranges=pcase.ranges_of(sb), pos_base=base, capacity=cap)
        return _rec_host(out, int(cnt.item())), (), None
    if family == "context":
        s = plan.scan_context(dev, before=pcase.CONTEXT_BEFORE, after=pcase.CONTEXT_AFTER, pos_base=base, capacity=cap)
        assert s.count == rec.size
        _same(_rec_host(s.records, s.count), moved(rec, base), (family, "the scan's records"))
        return None, _snippets(s), None
    if family == "replace":
        r = plan.scan_replace(dev, pcase.replacements_of(sb), pos_base=base, capacity=cap, out_start=True)
        sel = pcase.want_of(family, sb).rec
        _same(_rec_host(r.records, r.count), moved(sel, base), (family, "the selection"))
        return None, _replaced(r, sb, sel.size), None
    if family == "tokens":
        rest, start = _tokens(plan.scan_tokens(dev, mode="run", gap_base=pcase.TOKEN_GAP_BASE, pos_base=base, capacity=cap), False)
        return None, rest, start
    if family in ("patterns", "chains"):
        out, cnt, found, _ = (plan.scan_patterns if family == "patterns" else plan.scan_chains)(dev, tset, pos_base=base, capacity=cap)
        assert int(found.item()) == rec.size
        return _rec_host(out, int(cnt.item())), (), None
    fn = {"approx": plan.scan_approx, "edit": plan.scan_edit, "templates": plan.scan_templates}[family]
    out, dist, cnt, found, _ = fn(dev, tset, pos_base=base, capacity=cap)
    assert int(found.item()) == rec.size
    k = int(cnt.item())
    return _rec_host(out, k), (_np(dist, k, np.uint32),), None


def _host_form(family, sb, plan, base):
    """the family's *_host call (host memory in, blocking) at pos_base = base; None where the call takes no pos_base"""
    text = pcase.inputs(family, sb)[0]
    tset = _sets(family, sb, plan)
    if family == "select":
        return plan.scan_select_host(text, pos_base=base), (), None
    if family == "segment":
        out, sums = plan.scan_segment_host(text, pcase.SEGMENT_COST, pcase.SEGMENT_GAP, pos_base=base)
        return out, (np.array(sums, np.uint64),), None
    if family == "words":
        return plan.scan_words_host(text, ranges=pcase.ranges_of(sb), pos_base=base), (), None
    if family == "context":
        return None, _snippets(plan.scan_context_host(text, before=pcase.CONTEXT_BEFORE, after=pcase.CONTEXT_AFTER, pos_base=base)), None
    if family in ("replace", "tokens"):
        return None                                          # (acm_gpu_scan_replace_host and acm_gpu_scan_tokens_host take no pos_base)
    if family in ("patterns", "chains"):
        return (plan.scan_patterns_host if family == "patterns" else plan.scan_chains_host)(text, tset, pos_base=base), (), None
    fn = {"approx": plan.scan_approx_host, "edit": plan.scan_edit_host, "templates": plan.scan_templates_host}[family]
    out, dist = fn(text, tset, pos_base=base)
    return out, (dist,), None


def _family_cases():
    return [(f, sb) for f in pcase.FAMILIES for sb in ((1, 4) if f in pcase.TEXT_FAMILIES else (1,))]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family,sb", _family_cases())
def test_family_join_fused_and_host_forms_at_the_carry(torch_cuda, family, sb, name):
    """the carry inside an occurrence that the family's expected output holds (tests/test_positions_cpu.py shows the
    conditions): the join over the oracle's records, the fused scan, the host form; for the joins that take offsets
    with a base, a packed batch with the carry inside a text and one with the carry exactly on a text boundary"""
    m, plan = _machine(family, sb)
    c = pcase.boundary_of(family, sb)
    base = bases(c)[name]
    w = pcase.want_of(family, sb)
    pcase.same(_join(torch_cuda, family, sb, plan, moved(w.rec, base), base), w.at(base), (family, sb, name, "join"))
    pcase.same(_fused(torch_cuda, family, sb, plan, base), w.at(base), (family, sb, name, "fused"))
    got = _host_form(family, sb, plan, base)
    if got is not None:
        pcase.same(got, w.at(base), (family, sb, name, "host"))
    if family in pcase.BATCH_FAMILIES:
        n = pcase.inputs(family, sb)[0].size
        for off in (thirds(n), thirds(n, c)):
            cut = pcase.want_of(family, sb, off)
            pcase.same(_join(torch_cuda, family, sb, plan, moved(cut.rec, base), base, off), cut.at(base), (family, sb, name, off.tolist()))
    plan.status()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["tile64", "walk"])
def test_select_in_tiles_of_64_and_by_the_walk(torch_cuda, monkeypatch, mode, name):
    """tiles of 64 candidates: with c a few candidates in front of a tile seam the carry falls inside a tile, with c
    on the first candidate of a tile between two tiles; the walk form takes the same records"""
    monkeypatch.setenv("ACM_GPU_SELECT_TILE", "64")
    if mode == "walk":
        monkeypatch.setenv("ACM_GPU_SELECT", "walk")
    m, plan = _machine("select", 1)
    assert plan.select_form == (2 if mode == "walk" else 1)
    text, rec = pcase.inputs("select", 1)
    w = pcase.want_of("select", 1)
    starts = np.unique(extent(rec)[0])                                              # the candidates: distinct starts
    assert starts.size > 2 * 64
    inside = pcase.boundary_of("select", 1)
    seam = int(starts[64])                                                          # the first candidate of the second tile begins here
    assert np.searchsorted(starts, inside) % 64 not in (0, 63)
    for c in (inside, seam):
        base = bases(c)[name]
        out, k = plan.select_records(_rec_dev(torch_cuda, moved(rec, base)), rec.size, base, text.size)
        _same(_rec_host(out, k), moved(w.records, base), (mode, name, c))
        out, cnt, _ = plan.scan_select(_dev(torch_cuda, text), pos_base=base, capacity=rec.size)
        _same(_rec_host(out, int(cnt.item())), moved(w.records, base), (mode, name, c, "fused"))
    plan.status()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family", pcase.FAMILIES)
def test_a_wrong_high_word_is_seen_by_every_join(torch_cuda, family, name):
    """ONE stranger in a valid set: a position whose low word is that of a valid position and whose high word is
    wrong (in_range - 2^32, in_range + 2^32), pos_base - 1, pos_base + n_symbols.  acm_gpu_plan_status reports
    ACM_GPU_E_INTERNAL; select, segment, words, patterns, chains, approx, edit and templates drop the stranger and
    answer the rest, context, replace and tokens write nothing -- what each family's own test at pos_base 1000
    expects."""
    sb = 1
    m, _ = _machine(family, sb)
    c = pcase.boundary_of(family, sb)
    base = bases(c)[name]
    w = pcase.want_of(family, sb)
    text = pcase.inputs(family, sb)[0]
    good = moved(w.rec, base)
    model = good[good.size // 2]
    for pos in breach_positions(base, text.size, int(w.rec["end_pos"][w.rec.size // 2])):
        plan = m.plan(0)                                                            # (the error flag is sticky)
        plan.status()
        stranger = np.array([(pos, model["length"], model["keyword_id"])], po.RECORD_DTYPE)
        mixed = canonical(np.concatenate([good, stranger]))
        if family in ("replace", "tokens"):
            dev, d_rec = _dev(torch_cuda, text), _rec_dev(torch_cuda, mixed)
            if family == "replace":
                r = plan.replace_records(dev, d_rec, mixed.size, pcase.replacements_of(sb), pos_base=base)
                assert r.out_symbols == 0, (family, name, hex(pos))
            else:
                t = plan.tokens_records(dev, d_rec, mixed.size, mode="run", gap_base=pcase.TOKEN_GAP_BASE, pos_base=base)
                assert t.n_tokens == 0, (family, name, hex(pos))
        elif family == "context":
            s = plan.context_records(_dev(torch_cuda, text), _rec_dev(torch_cuda, mixed), mixed.size, before=pcase.CONTEXT_BEFORE, after=pcase.CONTEXT_AFTER,
                                     pos_base=base)
            assert (s.n_snippets, s.out_symbols) == (0, 0), (family, name, hex(pos))
        else:
            assert family in DROPS
            pcase.same(_join(torch_cuda, family, sb, plan, mixed, base), w.at(base), (family, name, hex(pos)))
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, (family, name, hex(pos))
        plan.close()
