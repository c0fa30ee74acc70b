"""The scratch a device call reports is the scratch it uses (acm_gpu_grep_device,
acm_gpu_tally_batch_device, acm_gpu_select_records_device, acm_gpu_words_records_device, the joins of
a record set under a compiled set -- acm_gpu_{patterns,chains,approx,edit,templates}_records_device --
and their fused forms acm_gpu_scan_{patterns,chains,approx}_device, called through binding.lib ()
directly).  With exactly *_tmp_bytes of room, every byte of it and of a
256-byte guard on either side set to 0xFF, a call gives what the matching Plan method gives (other
tests hold those against the oracle) and leaves both guards alone: nothing relies on scratch being
zero beyond what the call clears itself, and nothing is written past the reported size.  With one
byte less every call returns ACM_GPU_E_ARG and touches no output."""
import numpy as np
import pytest

from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import ANY, SymbolClass
from tests.batch_cases import packed_batch
from tests.cases import build_pair

pytestmark = pytest.mark.gpu

E_ARG = binding.ACM_GPU_E_ARG
KEYWORDS = [b"he", b"she", b"his", b"hers"]
N_SYMBOLS, N_TEXTS = 4096, 37
WINDOW, CAPACITY, PAIR_CAPACITY = 4096, 1024, 1024
GUARD, SENTINEL = 256, 0x5A
TERMS = ["patterns", "chains"]                      # joins that give records
SETS = ["approx", "edit", "templates"]              # joins that give records and a distance each
FUSED = {"scan_patterns": "patterns", "scan_chains": "chains", "scan_approx": "approx"}
FAMILIES = ["grep", "tally_batch", "select", "words"] + TERMS + SETS + list(FUSED)
OUT_ROOM = 1024                                     # matches a join has room for


def _sets():
    """a set per join family over the four keywords (he 0, she 1, his 2, hers 3), as the host description"""
    h, e, s, i, r = b"hesir"
    pieces = [[(0, 0, 2), (2, 2, 3)], [(1, 0, 3), (1, 3, 3)], [(3, 0, 4), (0, 4, 2)]]
    aset = binding.ApproxSet([b"hehis", b"sheshe", b"hershe"], 1, pieces)
    return {
        "patterns": binding.PatternSet([[(0, 0, 2), (0, 3, 2)], [(1, 0, 3), (0, 1, 2)], [(2, 0, 3), (0, 4, 2)], [(0, 0, 2), (2, 2, 3)]]),
        "chains": binding.ChainSet([[(0, 0, 0), (0, 0, 6)], [(1, 0, 0), (2, 0, 30)], [(2, 0, 0), (0, 1, 12), (3, 0, 40)]]),
        "approx": aset,
        "edit": aset,
        "templates": binding.TemplateSet([[h, e, ANY, h, i, s], [s, h, e, SymbolClass([i, r]), h, e], [h, i, s, SymbolClass([32], negate=True), ANY, h, e]],
                                         [0, 1, 1], [[(0, 0, 2), (2, 3, 3)], [(1, 0, 3), (0, 4, 2)], [(2, 0, 3), (0, 5, 2)]]),
    }


def _host_matches(family, rec, sets, text, off):
    """the matches of a join family by its definition on the host (acm_<family>_records)"""
    if family in TERMS:
        return getattr(binding, family + "_records")(rec, sets[family], N_SYMBOLS, offsets=off, n_keywords=len(KEYWORDS)).size
    return getattr(binding, family + "_records")(rec, sets[family], text, offsets=off, n_keywords=len(KEYWORDS))[0].size


def _batch():
    """tests/batch_cases.py::packed_batch: 4 KiB over a seven-letter alphabet, cut into 37 texts"""
    return packed_batch(N_SYMBOLS, N_TEXTS)


class Case:
    pass


@pytest.fixture(scope="module")
def case():
    """the plan, the batch on the device, the records of its ordered scan, a compiled set per join
    family and what the matching Plan methods give for them, made once"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    c = Case()
    c.torch = torch
    m, o = build_pair(KEYWORDS, 1)
    text, off = _batch()
    # on the CPU, by the oracle: enough matches for more than one tile or wave, all within the 1,024-record room
    whole = o.scan(text).size
    inside = sum(o.scan(text[int(off[t]):int(off[t + 1])]).size for t in range(N_TEXTS))
    assert 64 <= inside <= whole <= 1000, (inside, whole)
    c.machine, c.plan = m, m.plan(0)
    c.text = torch.from_numpy(text).cuda()
    c.offsets = torch.from_numpy(off.view(np.int64).copy()).cuda()
    c.ranges, c.n_ranges = binding._word_ranges(binding.ASCII_WORD, 1)
    rec, cnt, _ = c.plan.scan_ordered(c.text, capacity=CAPACITY)
    c.records, c.n = rec, int(cnt.item())
    assert c.n == whole
    g = c.plan.grep(c.text, c.offsets, window=WINDOW, capacity=CAPACITY)
    assert g.need <= CAPACITY and 0 < g.n_kept < N_TEXTS and g.out_symbols > 0
    tb = c.plan.tally_batch(c.text, c.offsets, window=WINDOW, capacity=CAPACITY, pair_capacity=PAIR_CAPACITY)
    assert tb.need <= CAPACITY and 0 < tb.nnz <= PAIR_CAPACITY and tb.total == inside
    sel, n_sel = c.plan.select_records(c.records, c.n, 0, N_SYMBOLS)
    assert 0 < n_sel < c.n
    wrd, n_wrd = c.plan.words_records(c.text, c.records, c.n, offsets=c.offsets)
    n_wrd = int(n_wrd.item())
    assert 0 < n_wrd < c.n
    # the joins: on the CPU, by the host definitions, none is trivial -- some matches, fewer than the output room
    sets = _sets()
    rec_host = o.scan(text)
    for family in TERMS + SETS:
        assert 0 < _host_matches(family, rec_host, sets, text, off) < OUT_ROOM, family
    c.sets = {"patterns": c.plan.patterns_create(sets["patterns"]), "chains": c.plan.chains_create(sets["chains"]),
              "approx": c.plan.approx_create(sets["approx"]), "templates": c.plan.templates_create(sets["templates"])}
    c.sets["edit"] = c.sets["approx"]
    joined = {}
    for family in TERMS:
        out, cnt = getattr(c.plan, family + "_records")(c.records, c.n, c.sets[family], N_SYMBOLS, offsets=c.offsets, out_capacity=OUT_ROOM)
        joined[family] = [out[:int(cnt.item())], cnt]
    for family in SETS:
        out, dist, cnt = getattr(c.plan, family + "_records")(c.records, c.n, c.sets[family], c.text, offsets=c.offsets, out_capacity=OUT_ROOM)
        joined[family] = [out[:int(cnt.item())], dist[:int(cnt.item())], cnt]
    for fused, family in FUSED.items():
        *outs, cnt, found, _ = getattr(c.plan, fused)(c.text, c.sets[family], offsets=c.offsets, capacity=CAPACITY, out_capacity=OUT_ROOM)
        joined[fused] = [t[:int(cnt.item())] for t in outs] + [torch.cat([cnt, found])]
        assert int(found.item()) == c.n and all(torch.equal(g, w) for g, w in zip(joined[fused][:-1], joined[family][:-1])), fused
    for family in TERMS + SETS:
        assert 0 < int(joined[family][-1].item()) < OUT_ROOM, family
    c.want = {
        **joined,
        "grep": [g.hits[:N_TEXTS], g.kept[:g.n_kept], torch.tensor([g.n_kept, g.total, g.need, g.out_symbols]), g.out[:g.out_symbols],
                 g.out_offsets[:g.n_kept + 1]],
        "tally_batch": [tb.row_ptr, tb.col[:tb.nnz], tb.val[:tb.nnz], torch.tensor([tb.nnz, tb.total, tb.need, tb.need_pairs])],
        "select": [sel[:n_sel], torch.tensor([n_sel])],
        "words": [wrd[:n_wrd], torch.tensor([n_wrd])],
    }
    torch.cuda.synchronize()
    return c


def _tmp_bytes(c, family):
    L, h = binding.lib(), c.plan.h
    if family == "grep":
        return L.acm_gpu_grep_tmp_bytes(h, WINDOW, CAPACITY, N_SYMBOLS, N_TEXTS)
    if family == "tally_batch":
        return L.acm_gpu_tally_batch_tmp_bytes(h, WINDOW, CAPACITY, PAIR_CAPACITY, N_SYMBOLS, N_TEXTS)
    if family == "select":
        return L.acm_gpu_select_tmp_bytes(h, c.n, N_SYMBOLS)
    if family in TERMS:
        return getattr(L, "acm_gpu_%s_tmp_bytes" % family)(h, c.sets[family].h, c.n, N_TEXTS)
    if family in SETS:
        return getattr(L, "acm_gpu_%s_tmp_bytes" % family)(h, c.sets[family].h, c.n, OUT_ROOM, N_TEXTS)
    if family == "scan_approx":
        return L.acm_gpu_scan_approx_tmp_bytes(h, c.sets["approx"].h, CAPACITY, OUT_ROOM, N_SYMBOLS, N_TEXTS)
    if family in FUSED:
        return getattr(L, "acm_gpu_%s_tmp_bytes" % family)(h, c.sets[FUSED[family]].h, CAPACITY, N_SYMBOLS, N_TEXTS)
    return L.acm_gpu_words_tmp_bytes(h, c.n, N_TEXTS)


def _outputs(c, family):
    """the call's output tensors, every byte SENTINEL"""
    torch = c.torch

    def full(n, dtype):
        t = torch.empty(n, dtype=dtype, device=c.text.device)
        t.view(torch.uint8).fill_(SENTINEL)
        return t
    if family == "grep":        # hits, kept, (n_kept, total, need, out_symbols), out, out_offsets
        return [full(N_TEXTS, torch.int64), full(N_TEXTS, torch.int32), full(4, torch.int64), full(N_SYMBOLS, torch.uint8),
                full(N_TEXTS + 1, torch.int64)]
    if family == "tally_batch":  # row_ptr, col, val, (nnz, total, need, need_pairs)
        return [full(N_TEXTS + 1, torch.int64), full(PAIR_CAPACITY, torch.int32), full(PAIR_CAPACITY, torch.int64), full(4, torch.int64)]
    if family in TERMS + SETS + list(FUSED):  # out, dist (the joins with a distance), count or (count, found)
        dist = [full(OUT_ROOM, torch.int32)] if family in SETS + ["scan_approx"] else []
        return [full(2 * OUT_ROOM, torch.int64).view(OUT_ROOM, 2)] + dist + [full(2 if family in FUSED else 1, torch.int64)]
    return [full(2 * c.n, torch.int64).view(c.n, 2), full(1, torch.int64)]   # out, count


def _call(c, family, out, d_tmp, tmp_bytes):
    L, h, st = binding.lib(), c.plan.h, c.plan._stream()
    p = [t.data_ptr() for t in out]
    if family == "grep":
        return L.acm_gpu_grep_device(h, c.text.data_ptr(), N_SYMBOLS, c.offsets.data_ptr(), N_TEXTS, binding.ACM_GREP_MATCHING, WINDOW, CAPACITY,
                                     p[0], p[1], p[2], p[2] + 8, p[2] + 16, p[3], N_SYMBOLS, p[4], p[2] + 24, d_tmp, tmp_bytes, st)
    if family == "tally_batch":
        return L.acm_gpu_tally_batch_device(h, c.text.data_ptr(), N_SYMBOLS, c.offsets.data_ptr(), N_TEXTS, WINDOW, CAPACITY, PAIR_CAPACITY,
                                            p[0], p[1], p[2], p[3], p[3] + 8, p[3] + 16, p[3] + 24, d_tmp, tmp_bytes, st)
    if family == "select":
        return L.acm_gpu_select_records_device(h, c.records.data_ptr(), c.n, None, 0, N_SYMBOLS, p[0], p[1], d_tmp, tmp_bytes, st)
    if family in TERMS:
        return getattr(L, "acm_gpu_%s_records_device" % family)(h, c.sets[family].h, c.records.data_ptr(), c.n, None, N_SYMBOLS, 0, c.offsets.data_ptr(),
                                                                N_TEXTS, p[0], OUT_ROOM, p[1], d_tmp, tmp_bytes, st)
    if family in SETS:
        return getattr(L, "acm_gpu_%s_records_device" % family)(h, c.sets[family].h, c.records.data_ptr(), c.n, None, c.text.data_ptr(), N_SYMBOLS, 0,
                                                                c.offsets.data_ptr(), N_TEXTS, p[0], p[1], OUT_ROOM, p[2], d_tmp, tmp_bytes, st)
    if family == "scan_approx":
        return L.acm_gpu_scan_approx_device(h, c.sets["approx"].h, c.text.data_ptr(), N_SYMBOLS, 0, c.offsets.data_ptr(), N_TEXTS, CAPACITY, p[0], p[1],
                                            OUT_ROOM, p[2], p[2] + 8, d_tmp, tmp_bytes, st)
    if family in FUSED:
        return getattr(L, "acm_gpu_%s_device" % family)(h, c.sets[FUSED[family]].h, c.text.data_ptr(), N_SYMBOLS, 0, c.offsets.data_ptr(), N_TEXTS, CAPACITY,
                                                        p[0], OUT_ROOM, p[1], p[1] + 8, d_tmp, tmp_bytes, st)
    return L.acm_gpu_words_records_device(h, c.text.data_ptr(), N_SYMBOLS, 0, c.offsets.data_ptr(), N_TEXTS, c.ranges.ctypes.data, c.n_ranges,
                                          binding.ACM_WORDS_BOTH, c.records.data_ptr(), c.n, None, p[0], p[1], d_tmp, tmp_bytes, st)


def _cut(family, out):
    """the part of every output that counts, as c.want lists it"""
    if family == "grep":
        n_kept, _, _, out_symbols = (int(x) for x in out[2].cpu())
        return [out[0], out[1][:n_kept], out[2], out[3][:out_symbols], out[4][:n_kept + 1]]
    if family == "tally_batch":
        nnz = int(out[3][0].item())
        return [out[0], out[1][:nnz], out[2][:nnz], out[3]]
    n = int(out[-1][0].item())                   # select, words and the joins: the count leads the last output
    return [t[:n] for t in out[:-1]] + [out[-1]]


@pytest.mark.parametrize("family", FAMILIES)
def test_exact_room(case, family):
    c, torch = case, case.torch
    tb = _tmp_bytes(c, family)
    assert tb > 0
    room = torch.empty(GUARD + tb + GUARD, dtype=torch.uint8, device=c.text.device)
    room.fill_(0xFF)
    out = _outputs(c, family)
    rc = _call(c, family, out, room.data_ptr() + GUARD, tb)
    torch.cuda.synchronize()
    assert rc == binding.ACM_GPU_OK, rc
    c.plan.status()                                      # (raises when a kernel flagged an error)
    got = _cut(family, out)
    assert len(got) == len(c.want[family])
    for i, (g, w) in enumerate(zip(got, c.want[family])):
        assert g.shape == w.shape and torch.equal(g.cpu(), w.cpu()), (family, i, g[:8], w[:8])
    assert bool((room[:GUARD] == 0xFF).all()), "written in front of d_tmp"
    assert bool((room[GUARD + tb:] == 0xFF).all()), "written past the reported size"


@pytest.mark.parametrize("family", FAMILIES)
def test_room_one_byte_short(case, family):
    c, torch = case, case.torch
    tb = _tmp_bytes(c, family)
    room = torch.empty(GUARD + tb + GUARD, dtype=torch.uint8, device=c.text.device)
    out = _outputs(c, family)
    rc = _call(c, family, out, room.data_ptr() + GUARD, tb - 1)
    torch.cuda.synchronize()
    assert rc == E_ARG, rc
    for i, t in enumerate(out):
        assert bool((t.view(torch.uint8) == SENTINEL).all()), (family, i)
