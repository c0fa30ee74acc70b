"""Shared by tests/test_cooccur_streams_gpu.py: a Case (tests/stream_cases.py) per device entry point of
include/acm_cooccur.h over a stream_cases.Features, with its expected value -- the brute force of the definition
(tests/cooccur_cases.py) over the oracle's count matrix, never the library's own scan.  Every entry point comes with the
flags that send it through the key-only sort (0) and through the pair sort and the running sum (PRODUCT; ADD always)."""
import numpy as np

from aho_corasick_1975_amd import binding
from tests import stream_cases as sc
from tests.cooccur_cases import DIAGONAL, PRODUCT, add_expected, brute_force, cut_rows

ENTRIES = ["acm_gpu_cooccur_matrix_device", "acm_gpu_cooccur_add_device", "acm_gpu_cooccur_device"]
# (entry point, flags): the key-only sort and the pair sort on the side stream
CASES = [("acm_gpu_cooccur_matrix_device", 0), ("acm_gpu_cooccur_matrix_device", PRODUCT | DIAGONAL), ("acm_gpu_cooccur_add_device", DIAGONAL),
         ("acm_gpu_cooccur_device", 0), ("acm_gpu_cooccur_device", PRODUCT)]
LIMIT = 6                                                # row_limit: some texts of the batch are skipped, most are not


def _pad(a, room):
    return np.concatenate([a, np.zeros(room - a.size, a.dtype)])


def _counts(f, rec):
    rp, c, v = f._matrix(rec)
    return rp.astype(np.uint64), c.astype(np.uint32), v.astype(np.uint64)


def _entries(e):
    return [e.co_ptr.astype(np.int64), e.co_col.view(np.int32), e.co_val.astype(np.int64)]


def expected(f, name, flags, which="real"):
    """the brute force over the oracle's count matrix, and the call's numbers where they have a definition"""
    e = brute_force(_counts(f, f._side(which)[1]), f.K, flags, LIMIT)
    if name == "acm_gpu_cooccur_matrix_device":
        return _entries(e) + [np.array([e.nnz, e.cross, e.skipped])]
    if name == "acm_gpu_cooccur_add_device":
        half = f.T // 2
        cn = _counts(f, f._side(which)[1])
        a, b = brute_force(cut_rows(cn, 0, half), f.K, flags, LIMIT), brute_force(cut_rows(cn, half, f.T), f.K, flags, LIMIT)
        return _entries(e) + [np.array([e.nnz, a.nnz + b.nnz])]
    return _entries(e) + [None]                          # (the counts of the windowed scan: a scratch diagnostic among them)


def case(torch, f, name, flags):
    L, h, N, T, K, CAP = binding.lib(), f.plan.h, f.N, f.T, f.K, sc.CAP
    counts, counts_decoy = _counts(f, f.rec), _counts(f, f.rec_decoy)
    want, other = brute_force(counts, K, flags, LIMIT), brute_force(counts_decoy, K, flags, LIMIT)
    # from the oracle alone: entries, a value of two or more, skipped texts and texts that contribute, and a decoy that differs
    assert want.nnz > 0 and int(want.co_val.max()) >= 2 and 0 < want.skipped < T and want.cross > 0
    assert not (np.array_equal(want.co_col, other.co_col) and np.array_equal(want.co_val, other.co_val))
    cross_room, out_room = max(want.cross, other.cross) + 3, max(want.nnz, other.nnz) + 3
    outs = {"co_ptr": (K + 1, torch.int64), "co_col": (out_room, torch.int32), "co_val": (out_room, torch.int64)}

    def cut(x, n):
        return [x["co_ptr"], x["co_col"][:n], x["co_val"][:n]]
    if name == "acm_gpu_cooccur_matrix_device":
        tb = L.acm_gpu_cooccur_matrix_tmp_bytes(h, T, K, cross_room)
        (rp, c, v), (rp2, c2, v2) = f._matrix(f.rec), f._matrix(f.rec_decoy)
        room = max(c.size, c2.size)
        return sc.Case("%s flags %d" % (name, flags), f.plan,
                       lambda p, st: L.acm_gpu_cooccur_matrix_device(h, p["row_ptr"], p["col"], p["val"], T, K, flags, LIMIT, cross_room, p["co_ptr"],
                                                                     p["co_col"], p["co_val"], out_room, p["res"], p["res"] + 8, p["res"] + 16, p["tmp"],
                                                                     tb, st),
                       {"row_ptr": (rp, rp2), "col": (_pad(c, room), _pad(c2, room)), "val": (_pad(v, room), _pad(v2, room))},
                       dict(outs, res=(3, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]], want=expected(f, name, flags))
    if name == "acm_gpu_cooccur_add_device":
        half = T // 2
        parts = [[brute_force(cut_rows(cn, 0, half), K, flags, LIMIT), brute_force(cut_rows(cn, half, T), K, flags, LIMIT)] for cn in (counts, counts_decoy)]
        assert all(p.nnz > 0 for pair in parts for p in pair)
        whole = add_expected(*parts[0])
        assert np.array_equal(whole.co_col, want.co_col) and np.array_equal(whole.co_val, want.co_val) and whole.nnz < parts[0][0].nnz + parts[0][1].nnz
        feed = max(p[0].nnz + p[1].nnz for p in parts)
        tb = L.acm_gpu_cooccur_add_tmp_bytes(h, K, feed)
        in_room = max(p.nnz for pair in parts for p in pair)
        gated = {}
        for i, side in enumerate(("a", "b")):
            real, decoy = parts[0][i], parts[1][i]
            gated[side + "_ptr"] = (real.co_ptr.astype(np.int64), decoy.co_ptr.astype(np.int64))
            gated[side + "_col"] = (_pad(real.co_col, in_room), _pad(decoy.co_col, in_room))
            gated[side + "_val"] = (_pad(real.co_val, in_room), _pad(decoy.co_val, in_room))
        return sc.Case("%s flags %d" % (name, flags), f.plan,
                       lambda p, st: L.acm_gpu_cooccur_add_device(h, p["a_ptr"], p["a_col"], p["a_val"], K, p["b_ptr"], p["b_col"], p["b_val"], K, feed,
                                                                  p["co_ptr"], p["co_col"], p["co_val"], out_room, p["res"], p["res"] + 8, p["tmp"], tb, st),
                       gated, dict(outs, res=(2, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]], want=expected(f, name, flags))
    tb = L.acm_gpu_cooccur_tmp_bytes(h, sc.WINDOW, CAP, CAP, N, T, K, cross_room)
    off = f.d_off.data_ptr()
    return sc.Case("%s flags %d" % (name, flags), f.plan,
                   lambda p, st: L.acm_gpu_cooccur_device(h, p["text"], N, off, T, sc.WINDOW, CAP, CAP, K, flags, LIMIT, cross_room, p["co_ptr"], p["co_col"],
                                                          p["co_val"], out_room, p["res"], p["res"] + 32, p["res"] + 40, p["res"] + 8, p["res"] + 16,
                                                          p["res"] + 24, p["tmp"], tb, st),
                   f._text(), dict(outs, res=(6, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]], want=expected(f, name, flags))
