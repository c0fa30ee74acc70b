"""Keywords of 64 to 9,000 symbols through every scan kernel family and on both sides of every place
where lmax (the longest keyword) changes what runs: dense rows up to 4081 and the CSR walk from 4082,
the one-pass tiled order and the tiled SELECT up to 1024, a bit more in sort keys and wire words at
64 / 128 / 256 ..., halos longer than a launch segment or a stream piece, a delta keyword longer than
every keyword of the base plan.  The cases are tests/long_cases.py's (test_long_keywords_cpu.py
checks them from the oracle alone); every comparison is bit-exact against oracle.pyoracle."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd.sharded import shard_bounds
from oracle import pyoracle as po
from tests import long_cases as lc
from tests.select_cases import greedy, nontrivial

pytestmark = pytest.mark.gpu

FORM_TILED, FORM_WALK = 1, 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _dev(torch, arr):
    a = np.ascontiguousarray(arr)
    a = a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.itemsize])
    return torch.from_numpy(a.copy()).cuda()


def _host(rec, n):
    return np.frombuffer(rec[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()


def _same(got, want, what=""):
    assert got.size == want.size and np.array_equal(got, want), (what, got.size, want.size)


def _plan(monkeypatch, name, extra_env=None):
    """the case's plan, made under the case's switches, of the family the case is meant for"""
    for k in ("ACM_GPU_GRAM", "ACM_GPU_GRAM2", "ACM_GPU_SPARSE", "ACM_GPU_SEGMENT_LOG2", "ACM_GPU_ORDER", "ACM_GPU_SELECT",
              "ACM_GPU_SELECT_TILE", "ACM_GPU_DELTA", "ACM_GPU_GRID_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in {**lc.CASES[name][1], **(extra_env or {})}.items():
        monkeypatch.setenv(k, v)
    m = lc.machine(name)
    plan = m.plan(0)
    lc.assert_family(name, plan.info)
    assert m.lmax == lc.params(name)["lmax"]
    return m, plan


MATRIX = [n for n in sorted(lc.CASES) if not n.endswith(("-seams", "-short"))]
# one case per family (the largest lmax that is a matrix case of all of them: past the tiled order)
FAMILIES = ["dense-1025", "sticky-256", "csr-4082", "gram2-1025", "gram2short-1025", "gramold-1025", "hashed-1025",
            "starts16-1025", "starts32-1025", "walk16-1025", "walk32-1025"]
# ... and both sides of every lmax at which the sort keys' length field gains a bit, up to the widest one
LENGTH_BITS = ["dense-64", "dense-65", "dense-255", "dense-256", "dense-1024", "gram2-64", "gram2-1024", "gram2-4081", "csr-9000"]


@pytest.mark.parametrize("name", MATRIX)
def test_family_at_lmax(torch_cuda, monkeypatch, name):
    """every entry point of a whole scan: ordered in one call, scan + count read back + order, count-only,
    host buffers in and out"""
    m, plan = _plan(monkeypatch, name)
    kws, text = lc.case(name)
    o, want = lc.answer(name)
    dev = _dev(torch_cuda, text)
    _same(plan.scan_sorted(dev), want, "fused")
    _same(plan.scan_sorted(dev, fused=False), want, "scan, then order")
    assert int(plan.count(dev).item()) == want.size
    _same(plan.scan_host(text), want, "scan_host")
    plan.status()


@pytest.mark.parametrize("name", FAMILIES + LENGTH_BITS)
def test_family_radix_order(torch_cuda, monkeypatch, name):
    """ACM_GPU_ORDER=radix: the sort keys carry len_bits_of (lmax) bits of length"""
    m, plan = _plan(monkeypatch, name, {"ACM_GPU_ORDER": "radix"})
    _, want = lc.answer(name)
    dev = _dev(torch_cuda, lc.case(name)[1])
    _same(plan.scan_sorted(dev), want, "fused")
    _same(plan.scan_sorted(dev, fused=False), want, "scan, then order")
    plan.status()


@pytest.mark.parametrize("name", ["starts16-1025", "starts32-1025", "walk16-1025", "walk32-1025"])
def test_buffer_that_is_not_16_byte_aligned(torch_cuda, monkeypatch, name):
    m, plan = _plan(monkeypatch, name)
    kws, text = lc.case(name)
    o, _ = lc.answer(name)
    dev = _dev(torch_cuda, text)
    assert dev[1:].data_ptr() % 16 != 0
    want = o.scan(text[1:])
    assert (want["length"] == m.lmax).sum() >= 100
    _same(plan.scan_sorted(dev[1:]), want)
    assert int(plan.count(dev[1:]).item()) == want.size
    plan.status()


# ---- cuts and seams

CUT_CASES = ["dense-1025", "gram2-1025", "starts32-1025", "csr-4082"]


@pytest.mark.parametrize("name", CUT_CASES)
def test_emit_from_inside_and_just_behind_a_long_match(torch_cuda, monkeypatch, name):
    m, plan = _plan(monkeypatch, name)
    kws, text = lc.case(name)
    o, want = lc.answer(name)
    lmax = m.lmax
    dev = _dev(torch_cuda, text)
    ends = lc.spine_ends(name)
    e = int(ends[ends.size // 2])
    spine = np.array([(e, lmax, 0)], po.RECORD_DTYPE)
    for base in (0, 1 << 40):
        for cut, reported in ((e - lmax // 2, True), (e + 1, False)):     # the match starts before either cut
            ref = o.scan(text, pos_base=base, emit_from=cut)
            sel = want[want["end_pos"] >= cut].copy()
            sel["end_pos"] += base
            assert np.array_equal(ref, sel)
            shifted = spine.copy()
            shifted["end_pos"] += base
            assert bool(np.isin(shifted, ref)[0]) == reported
            _same(plan.scan_sorted(dev, emit_from=cut, pos_base=base), ref, (base, cut))
            _same(plan.scan_sorted(dev, emit_from=cut, pos_base=base, fused=False), ref, (base, cut, "scan, then order"))
        assert int(plan.count(dev, emit_from=e + 1).item()) == int((want["end_pos"] > e).sum())
    plan.status()


def _shards(torch, plan, dev, n, lmax, world=4):
    """the records of `world` shards side by side, each scanned from lmax - 1 symbols before its own
    range (a copy of the slice: 16-byte aligned whatever lmax, so the plan's own kernel takes it)"""
    parts = []
    for r in range(world):
        rb, b, e = shard_bounds(n, r, world, lmax)
        assert rb == max(b - (lmax - 1), 0)
        parts.append(plan.scan_sorted(dev[rb:e].clone(), emit_from=b - rb, pos_base=rb))
    return np.concatenate(parts)


@pytest.mark.parametrize("name", CUT_CASES)
def test_four_shards_equal_the_whole(torch_cuda, monkeypatch, name):
    m, plan = _plan(monkeypatch, name)
    _, want = lc.answer(name)
    n, lmax = lc.params(name)["n"], m.lmax
    ends = lc.spine_ends(name)
    cuts = np.array([n * r // 4 for r in range(1, 4)])
    assert ((ends[:, None] >= cuts) & (ends[:, None] - lmax + 1 < cuts)).any(), "no S across a shard cut"
    assert np.isin(ends, cuts).any(), "no S that ends on the first symbol of a shard (its start is the shard's read_begin)"
    _same(_shards(torch_cuda, plan, _dev(torch_cuda, lc.case(name)[1]), n, lmax), want)
    plan.status()


@pytest.mark.parametrize("name,seg_log2", lc.SEAM_CASES)
def test_launch_segments_shorter_than_or_near_the_halo(torch_cuda, monkeypatch, name, seg_log2):
    """segments of 2^12 symbols under a halo of 4,999 (two seams inside one keyword) or 4,080, and
    of 2^16 symbols under a halo of 1,024 (4,081 for the CSR walk): records, count-only, emit_from"""
    m, plan = _plan(monkeypatch, name, {"ACM_GPU_SEGMENT_LOG2": str(seg_log2)})
    _, want = lc.answer(name)
    ends = lc.spine_ends(name)
    assert lc.seams_crossed(name, seg_log2).max() >= (2 if m.lmax > (1 << seg_log2) else 1)
    assert (ends % (1 << seg_log2) == 0).any(), "no S that ends on the first symbol of a segment: the whole halo is needed"
    dev = _dev(torch_cuda, lc.case(name)[1])
    _same(plan.scan_sorted(dev), want, "records")
    assert int(plan.count(dev).item()) == want.size
    cut = int(ends[ends.size // 2]) - 7
    _same(plan.scan_sorted(dev, emit_from=cut), want[want["end_pos"] >= cut], "emit_from")
    plan.status()


# ---- the one-pass tiled order: 1024 is the last lmax that takes it

@pytest.mark.parametrize("name", ["gram2-1024", "gram2-1025"])
def test_scan_ordered_exact_and_half_capacity(torch_cuda, monkeypatch, name):
    m, plan = _plan(monkeypatch, name)
    _, want = lc.answer(name)
    dev = _dev(torch_cuda, lc.case(name)[1])
    rec, cnt, _ = plan.scan_ordered(dev, capacity=want.size)
    assert int(cnt.item()) == want.size and rec.shape[0] == want.size
    _same(_host(rec, want.size), want, "exact capacity")
    half = want.size // 2
    rec, cnt, _ = plan.scan_ordered(dev, capacity=half)
    assert int(cnt.item()) == want.size and rec.shape[0] == half      # the full total, nothing past the end
    _same(plan.scan_sorted(dev, capacity=half), want, "grown and repeated")
    plan.status()


# ---- streaming: pieces shorter than the keyword (the halo in front of a piece spans several pieces)

@pytest.mark.parametrize("name,piece", [("dense-4081", 1000), ("dense-4081", 1024), ("dense-65-short", 7), ("dense-65-short", 8),
                                        ("gram2-4081", 1024), ("starts32-5000", 1024)])
def test_stream_pieces_shorter_than_the_keyword(torch_cuda, monkeypatch, name, piece):
    """pieces of 1,000 and of 7 symbols; of 1,024 and of 8 as well: an S then ends on the first symbol
    of a piece, and the context in front of that piece has to be all of lmax - 1 symbols"""
    m, plan = _plan(monkeypatch, name)
    o, want = lc.answer(name)
    text = lc.case(name)[1]
    assert piece < m.lmax
    assert piece not in (8, 1024) or (lc.spine_ends(name) % piece == 0).any()
    stream = plan.stream(max_piece_symbols=piece, record_capacity=want.size + 16)
    for off in range(0, text.size, piece):
        stream.feed(text[off:off + piece])
    got = stream.finish()
    stream.close()
    _same(got, want)
    plan.status()


# ---- a delta keyword longer than every keyword of the base plan

@pytest.mark.parametrize("name", ["dense-64", "gram2-64"])
def test_delta_keyword_longer_than_the_base_plans(torch_cuda, monkeypatch, name):
    m, plan = _plan(monkeypatch, name)
    p = lc.params(name)
    n = p["n"]
    kws, text = lc.case(name)
    rng = np.random.default_rng(77)
    K = rng.integers(p["lo"], p["lo"] + p["span"], size=1500).astype(text.dtype)
    text = text.copy()
    tile = 64 * 2 * 64      # the dense kernel's wave tile (8 KiB); 4-gram tiles are multiples of 1 KiB groups
    for at in (5 * tile - 700, n // 4 - 800, 3 * n // 4 - 1499, n // 2 + 3 * tile + 1024 - 1):
        text[at:at + K.size] = K
    o = po.Oracle(p["sym"], po.AC75)
    for w in kws + [K]:
        o.add_keyword(w)
    want = o.scan(text)
    long_ends = want["end_pos"][want["length"] == 1500].astype(np.int64)
    assert long_ends.size == 4 and o.lmax == 1500
    dev = _dev(torch_cuda, text)
    base_kernel = plan.info.kernel
    _same(plan.scan_sorted(dev), want[want["length"] < 1500], "before the update")
    m.add_keyword(K)
    plan.update(m)
    assert plan.info.delta_keywords == 1 and plan.info.merges == 0 and plan.info.kernel == base_kernel
    assert m.lmax == 1500
    _same(plan.scan_sorted(dev), want, "fused")
    _same(plan.scan_sorted(dev, fused=False), want, "scan, then order")
    rec, cnt, _ = plan.scan_ordered(dev, capacity=want.size)
    assert int(cnt.item()) == want.size
    _same(_host(rec, want.size), want, "exact capacity")
    assert int(plan.count(dev).item()) == want.size
    _same(plan.scan_host(text), want, "scan_host")
    _same(_shards(torch_cuda, plan, dev, n, m.lmax), want, "shards")
    cut = int(long_ends[1]) - 3
    _same(plan.scan_sorted(dev, emit_from=cut, pos_base=1 << 40), o.scan(text, pos_base=1 << 40, emit_from=cut), "emit_from")
    plan.status()


# ---- consumers whose form depends on lmax

@pytest.mark.parametrize("name,form", [("dense-1024", FORM_TILED), ("dense-1025", FORM_WALK), ("dense-2049", FORM_WALK),
                                       ("gram2-1024", FORM_TILED), ("gram2-1025", FORM_WALK)])
def test_select_tiled_up_to_1024_walk_beyond(torch_cuda, monkeypatch, name, form):
    m, plan = _plan(monkeypatch, name)
    _, rec = lc.answer(name)
    want = greedy(rec)
    nontrivial(rec, want)
    assert (want["length"] == m.lmax).sum() >= 3
    assert plan.select_form == form
    dev = _dev(torch_cuda, lc.case(name)[1])
    out, cnt, _ = plan.scan_select(dev, capacity=rec.size)
    k = int(cnt.item())
    assert k == want.size
    _same(_host(out, k), want, "scan_select")
    _same(plan.scan_select_host(lc.case(name)[1]), want, "scan_select_host")
    plan.status()


@pytest.mark.parametrize("name,len_bits", [("dense-255", 8), ("dense-256", 9), ("csr-9000", 14)])
def test_wire_words_round_trip(torch_cuda, monkeypatch, name, len_bits):
    torch = torch_cuda
    m, plan = _plan(monkeypatch, name)
    _, want = lc.answer(name)
    n = lc.params(name)["n"]
    dev = _dev(torch, lc.case(name)[1])
    for base in (0, (1 << 41) + 4096):
        wire = plan.wire(n, base)
        assert wire == (base, 18, len_bits)
        rec, cnt, _ = plan.scan_ordered(dev, pos_base=base, capacity=want.size)
        assert int(cnt.item()) == want.size
        shifted = want.copy()
        shifted["end_pos"] += base
        _same(_host(rec, want.size), shifted, "ordered")
        packed = acm.binding.pack_records(rec[:want.size], wire)
        assert packed.shape == (want.size,) and packed.dtype == torch.int64
        back = torch.zeros((want.size, 2), dtype=torch.int64, device="cuda")
        acm.binding.unpack_records(packed, wire, back)
        assert torch.equal(back, rec[:want.size])
        _same(_host(back, want.size), shifted, "unpacked")
    plan.status()
