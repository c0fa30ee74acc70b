"""Dense kernel, continuation mode: a lane runs a fixed number of steps past its 64-byte chunk, and
a lane-stream still inside a match after them parks one walk item that the expand kernel finishes
through the HBM rows.  Texts and dictionaries that leave lanes inside matches at chunk and tile
ends, against the CPU oracle (records, count-only, digests)."""
import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from tests.cases import build_pair

pytestmark = pytest.mark.gpu

CHUNK = 64                 # bytes per lane-stream chunk
TILE = 64 * 2 * CHUNK      # bytes per wave tile (64 lanes x 2 streams)
AZ = np.arange(97, 123, dtype=np.uint8)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _check(torch, m, o, text, kernel=1, entry_bytes=2):
    plan = m.plan(0)
    assert plan.info.kernel == kernel and plan.info.entry_bytes == entry_bytes, plan.describe()
    dev = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    want = o.scan(text)
    got = plan.scan_sorted(dev)
    assert got.size == want.size and np.array_equal(got, want)
    assert int(plan.count(dev).item()) == want.size
    return want.size


def _plant_across(rng, text, kws, stride):
    """every `stride` bytes, a keyword that starts before the boundary and ends after it"""
    for b in range(stride, text.size - 64, stride):
        w = np.frombuffer(kws[int(rng.integers(0, len(kws)))], np.uint8)
        s = b - int(rng.integers(1, w.size))
        text[s:s + w.size] = w
    return text


def _long_keywords(rng, count, lo=20, hi=60):
    return [bytes(rng.choice(AZ, size=int(rng.integers(lo, hi + 1)))) for _ in range(count)]


def test_long_keywords_across_chunk_and_tile_ends(torch_cuda):
    rng = np.random.default_rng(11)
    kws = _long_keywords(rng, 40)
    kws += [w[:k] for w in kws[:10] for k in (2, 3, 4, 5, 9)]   # outputs on the way down a long match
    m, o = build_pair(kws, 1)
    text = rng.choice(AZ, size=9 * TILE + 37)
    _plant_across(rng, text, kws, TILE)
    _plant_across(rng, text, kws, 3 * CHUNK)
    # near misses: a long prefix that dies a few symbols past the chunk end
    for b in range(CHUNK * 5, text.size - 64, CHUNK * 11):
        w = np.frombuffer(kws[int(rng.integers(0, 40))], np.uint8)
        s = b - 2
        text[s:s + w.size - 1] = w[:-1]
        text[s + w.size - 1] = 96
    assert _check(torch_cuda, m, o, text) > 100


def test_every_chunk_ends_inside_a_match(torch_cuda):
    rng = np.random.default_rng(12)
    s = bytes(rng.choice(AZ, size=50))
    m, o = build_pair([s, s[10:30], s[:7], s[45:] + s[:20]], 1)
    text = np.frombuffer(s * (4 * TILE // 50 + 3), np.uint8)[: 4 * TILE + 5].copy()
    assert _check(torch_cuda, m, o, text) > 4 * TILE // 50
    # one symbol: every position ends keywords of several lengths, every lane is deep at every chunk end
    m, o = build_pair([b"a" * k for k in (1, 4, 5, 17, 33, 40)], 1)
    text = np.full(2 * TILE + 3, 97, np.uint8)
    _check(torch_cuda, m, o, text)


@pytest.mark.parametrize("lmax", [1, 2, 3, 4, 5, 6, 9])
def test_lmax_around_the_runover_length(torch_cuda, lmax):
    """lmax up to the run-over length never parks a walk item, lmax above it does"""
    rng = np.random.default_rng(100 + lmax)
    ab = np.array([97, 98], np.uint8)
    kws = {bytes(rng.choice(ab, size=int(rng.integers(1, lmax + 1)))) for _ in range(12)}
    kws |= {b"a" * lmax, b"ab" * (lmax // 2) + b"a" * (lmax % 2)}
    m, o = build_pair(sorted(kws), 1)
    text = rng.choice(ab, size=4 * TILE + 13)
    assert _check(torch_cuda, m, o, text) > 0


@pytest.mark.parametrize("blocks", [1, 17])
def test_small_grids(torch_cuda, monkeypatch, blocks):
    monkeypatch.setenv("ACM_GPU_GRID_BLOCKS", str(blocks))
    rng = np.random.default_rng(13)
    kws = _long_keywords(rng, 30) + [bytes(rng.choice(AZ, size=4)) for _ in range(200)]
    m, o = build_pair(kws, 1)
    text = rng.choice(AZ, size=70 * TILE + 101)
    _plant_across(rng, text, kws[:30], TILE)
    _plant_across(rng, text, kws[:30], 5 * CHUNK + 1)
    plan = m.plan(0)
    assert plan.info.grid_blocks == blocks
    assert _check(torch_cuda, m, o, text) > 1000


def test_count_only_and_records_across_segment_seams(torch_cuda, monkeypatch):
    """config 2's dictionary with long keywords added, segments of 64 KiB (walk items next to the
    end of a segment), records and count-only against the oracle's count and digest"""
    monkeypatch.setenv("ACM_GPU_SEGMENT_LOG2", "16")
    rng = np.random.default_rng(14)
    kd, ko = acm.synth.keywords(1000)
    kws = [bytes(kd[ko[i]:ko[i + 1]]) for i in range(1000)] + _long_keywords(rng, 20)
    m, o = build_pair(kws, 1)
    n = 4 << 20
    text = acm.synth.text(n, kd, ko).copy()
    _plant_across(rng, text, kws[1000:], 1 << 16)
    _plant_across(rng, text, kws[1000:], TILE + CHUNK)
    want_n, want_d = o.scan_mt(text, 8)
    plan = m.plan(0)
    assert plan.info.kernel == 1
    dev = torch_cuda.from_numpy(text).cuda()
    rec, cnt = plan.scan(dev, capacity=want_n + 16)
    assert acm.synth.device_digest(rec, int(cnt.item())) == (want_n, want_d)
    assert int(plan.count(dev).item()) == want_n


def test_sticky_mode_more_than_32768_states(torch_cuda, monkeypatch):
    """u32 states (the dense walk, not the 4-gram kernel): its slow side parks straight into HBM too"""
    monkeypatch.setenv("ACM_GPU_GRAM", "0")
    rng = np.random.default_rng(15)
    kws = [bytes(rng.choice(AZ, size=int(rng.integers(4, 13)))) for _ in range(6000)] + _long_keywords(rng, 20)
    m, o = build_pair(kws, 1)
    text = rng.choice(AZ, size=16 * TILE + 7)
    _plant_across(rng, text, kws, 997)
    _plant_across(rng, text, kws[6000:], CHUNK * 3)
    assert m.plan(0).info.dense_rows > 32768
    assert _check(torch_cuda, m, o, text, entry_bytes=4) > 100
