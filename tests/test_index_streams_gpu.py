"""The three device entry points of include/acm_index.h on a stream that is not the default one: the EARLY / LATE /
CONTROL arrangements of tests/stream_cases.py (Gates, Case, exercise), over the dense batch of tests/test_streams_gpu.py,
with ACM_GPU_INDEX_LIST between the batch's list lengths so that the one-wave sort and the wide form's radix sort both run
on the side stream.  The expected value is the plain call's on the null stream, held here against the brute-force
transposition of the oracle's count matrix (tests/index_cases.py) as well."""
import os

import numpy as np
import pytest

from aho_corasick_1975_amd import binding
from tests import stream_cases as sc
from tests.cases import build_pair
from tests.index_cases import brute_force, concat_expected, cut_rows, forms_of
from tests.test_scratch_bounds_gpu import KEYWORDS, _batch
from tests.test_streams_gpu import _decoy_batch

HEADER = os.path.join(sc.ROOT, "include", "acm_index.h")
ENTRIES = ["acm_gpu_index_matrix_device", "acm_gpu_index_concat_device", "acm_gpu_index_device"]
BASE = 1000


def test_every_stream_entry_point_of_the_header_is_exercised():
    assert sorted(sc.header_stream_functions(path=HEADER)) == sorted(ENTRIES)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def gates(torch_cuda):
    return sc.Gates(torch_cuda)


@pytest.fixture(scope="module")
def features(torch_cuda):
    text, off = _batch()
    m, o = build_pair(KEYWORDS, 1)
    return sc.Features(torch_cuda, m, o, m.plan, text, _decoy_batch(), off)


def _counts(f, rec):
    rp, c, v = f._matrix(rec)
    return rp.astype(np.uint64), c.astype(np.uint32), v.astype(np.uint64)


def _pad(a, room):
    return np.concatenate([a, np.zeros(room - a.size, a.dtype)])


def _wants(e):
    return [e.post_ptr.astype(np.int64), e.post_text.view(np.int32), e.post_count.astype(np.int64)]


def _longest(f):
    """a value of ACM_GPU_INDEX_LIST with lists of the real batch on either side of it"""
    lengths = np.unique(brute_force(_counts(f, f.rec), f.K).df)
    lengths = lengths[lengths > 0]
    assert lengths.size >= 2
    return int(lengths[(lengths.size - 1) // 2])


def _case(torch, f, name, longest):
    L, h, N, T, K, CAP = binding.lib(), f.plan.h, f.N, f.T, f.K, sc.CAP
    counts, counts_decoy = _counts(f, f.rec), _counts(f, f.rec_decoy)
    want, other = brute_force(counts, K, BASE), brute_force(counts_decoy, K, BASE)
    fast, wide = forms_of(want, longest)
    assert fast > 0 and wide > 0 and T > longest and max(want.nnz, other.nnz) <= CAP
    outs = {"post_ptr": (K + 1, torch.int64), "post_text": (CAP, torch.int32), "post_count": (CAP, torch.int64)}

    def cut(x, n):
        return [x["post_ptr"], x["post_text"][:n], x["post_count"][:n]]
    if name == "acm_gpu_index_matrix_device":
        tb = L.acm_gpu_index_matrix_tmp_bytes(h, T, K, CAP)
        (rp, c, v), (rp2, c2, v2) = f._matrix(f.rec), f._matrix(f.rec_decoy)
        room = max(c.size, c2.size)
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_index_matrix_device(h, p["row_ptr"], p["col"], p["val"], T, K, BASE, p["post_ptr"], p["post_text"],
                                                                   p["post_count"], CAP, p["res"], p["res"] + 8, p["tmp"], tb, st),
                       {"row_ptr": (rp, rp2), "col": (_pad(c, room), _pad(c2, room)), "val": (_pad(v, room), _pad(v2, room))},
                       dict(outs, res=(3, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]],
                       want=_wants(want) + [np.array([want.nnz, fast, wide])])
    if name == "acm_gpu_index_concat_device":
        half = T // 2
        parts = [[brute_force(cut_rows(cn, 0, half), K, BASE), brute_force(cut_rows(cn, half, T), K, BASE + half)] for cn in (counts, counts_decoy)]
        assert all(p.nnz > 0 for pair in parts for p in pair)
        assert np.array_equal(concat_expected(*parts[0]).post_text, want.post_text)
        tb = L.acm_gpu_index_concat_tmp_bytes(h, K)
        gated = {}
        for i, side in enumerate(("a", "b")):
            real, decoy = parts[0][i], parts[1][i]
            gated[side + "_ptr"] = (real.post_ptr.astype(np.int64), decoy.post_ptr.astype(np.int64))
            gated[side + "_text"] = (_pad(real.post_text, CAP), _pad(decoy.post_text, CAP))
            gated[side + "_count"] = (_pad(real.post_count, CAP), _pad(decoy.post_count, CAP))
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_index_concat_device(h, p["a_ptr"], p["a_text"], p["a_count"], K, p["b_ptr"], p["b_text"], p["b_count"], K,
                                                                   p["post_ptr"], p["post_text"], p["post_count"], CAP, p["res"], p["tmp"], tb, st),
                       gated, dict(outs, res=(1, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]],
                       want=_wants(want) + [np.array([want.nnz])])
    tb = L.acm_gpu_index_tmp_bytes(h, sc.WINDOW, CAP, CAP, N, T, K, CAP)
    off = f.d_off.data_ptr()
    return sc.Case(name, f.plan,
                   lambda p, st: L.acm_gpu_index_device(h, p["text"], N, off, T, sc.WINDOW, CAP, CAP, K, BASE, p["post_ptr"], p["post_text"], p["post_count"],
                                                        CAP, p["res"], p["res"] + 32, p["res"] + 8, p["res"] + 16, p["res"] + 24, p["tmp"], tb, st),
                   f._text(), dict(outs, res=(6, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]], want=_wants(want) + [None])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_index_entry_points_on_a_side_stream(torch_cuda, monkeypatch, gates, features, entry):
    longest = _longest(features)
    monkeypatch.setenv("ACM_GPU_INDEX_LIST", str(longest))
    bad = sc.exercise(torch_cuda, gates, _case(torch_cuda, features, entry, longest), control=entry == "acm_gpu_index_device")
    assert not bad, "\n".join(bad)
