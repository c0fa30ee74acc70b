"""The three device entry points of include/acm_score.h on a stream that is not the default one: the EARLY / LATE /
CONTROL arrangements of tests/stream_cases.py (Gates, Case, exercise), over the dense batch of tests/test_streams_gpu.py.
The expected value is the plain call's on the null stream, held here against the brute-force evaluation of the oracle's
count matrix (tests/score_cases.py) as well."""
import os

import numpy as np
import pytest

from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import score_class, weight
from tests import stream_cases as sc
from tests.cases import build_pair
from tests.score_cases import expected_scored
from tests.test_scratch_bounds_gpu import KEYWORDS, _batch
from tests.test_streams_gpu import _decoy_batch

HEADER = os.path.join(sc.ROOT, "include", "acm_score.h")
ENTRIES = ["acm_gpu_score_matrix_device", "acm_gpu_score_top_device", "acm_gpu_score_device"]
TOP = 4


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


def _model(f):
    """over the two keywords the real batch holds most often (the ones f.ruleset is made of)"""
    a, b = int(f.ruleset.terms[0][0]), int(f.ruleset.terms[1][0])
    return binding.ScoreModel([score_class([weight(a, 3), weight(b, -2)]), score_class([weight(b, 2, 2)], threshold=2),
                               score_class([weight(a, -1)], bias=1), score_class([weight(a, 1), weight(b, 1)], threshold=3)])


def _expected(f, rec, sm):
    rp, c, v = f._matrix(rec)
    return expected_scored((rp.astype(np.uint64), c.astype(np.uint32), v.astype(np.uint64)), sm)


def _pad(a, room):
    return np.concatenate([a, np.zeros(room - a.size, a.dtype)])


def _case(torch, f, name):
    L, h, N, T, CAP = binding.lib(), f.plan.h, f.N, f.T, sc.CAP
    sm = _model(f)
    if "score" not in f.handles:
        f.handles["score"] = f.plan.score_create(sm)
    S = f.handles["score"].h
    C = sm.n_classes
    FC = T * C
    want, other = _expected(f, f.rec, sm), _expected(f, f.rec_decoy, sm)
    assert 0 < want.n_kept <= FC and want.n_kept != other.n_kept
    top_n, top_text, top_score = want.top(TOP)
    kept_outs = {"kept_ptr": (T + 1, torch.int64), "kept_class": (FC, torch.int32), "kept_score": (FC, torch.int64), "best": (T, torch.int32)}
    top_outs = {"hits": (C, torch.int64), "top_n": (C, torch.int32), "top_text": (C * TOP, torch.int32), "top_score": (C * TOP, torch.int64)}
    kept_want = [want.kept_ptr.astype(np.int64), want.kept_class.view(np.int32), want.kept_score, want.best.view(np.int32)]
    top_want = [want.class_hits.astype(np.int64), top_n.view(np.int32), top_text.reshape(-1).view(np.int32), top_score.reshape(-1)]

    def kept_cut(x, n):
        return [x["kept_ptr"], x["kept_class"][:n], x["kept_score"][:n], x["best"]]

    def top_cut(x):
        return [x["hits"], x["top_n"], x["top_text"], x["top_score"]]
    if name == "acm_gpu_score_matrix_device":
        tb = L.acm_gpu_score_matrix_tmp_bytes(h, S, T)
        (rp, c, v), (rp2, c2, v2) = f._matrix(f.rec), f._matrix(f.rec_decoy)
        room = max(c.size, c2.size)
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_score_matrix_device(h, S, p["row_ptr"], p["col"], p["val"], T, p["kept_ptr"], p["kept_class"], p["kept_score"],
                                                                   FC, p["n_kept"], p["best"], p["tmp"], tb, st),
                       {"row_ptr": (rp, rp2), "col": (_pad(c, room), _pad(c2, room)), "val": (_pad(v, room), _pad(v2, room))},
                       dict(kept_outs, n_kept=(1, torch.int64)), tb, cut=lambda x: kept_cut(x, x["n_kept"][0]) + [x["n_kept"]],
                       want=kept_want + [np.array([want.n_kept])])
    if name == "acm_gpu_score_top_device":
        tb = L.acm_gpu_score_top_tmp_bytes(h, FC, C)
        gated = {"kept_ptr": (want.kept_ptr.astype(np.int64), other.kept_ptr.astype(np.int64)),
                 "kept_class": (_pad(want.kept_class, FC), _pad(other.kept_class, FC)), "kept_score": (_pad(want.kept_score, FC), _pad(other.kept_score, FC))}
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_score_top_device(h, p["kept_ptr"], p["kept_class"], p["kept_score"], FC, T, C, TOP, p["hits"], p["top_n"],
                                                                p["top_text"], p["top_score"], p["tmp"], tb, st),
                       gated, top_outs, tb, cut=top_cut, want=top_want)
    tb = L.acm_gpu_score_tmp_bytes(h, S, sc.WINDOW, CAP, CAP, N, T, FC, TOP)
    off = f.d_off.data_ptr()
    return sc.Case(name, f.plan,
                   lambda p, st: L.acm_gpu_score_device(h, S, p["text"], N, off, T, sc.WINDOW, CAP, CAP, p["kept_ptr"], p["kept_class"], p["kept_score"], FC,
                                                        p["res"], p["best"], TOP, p["hits"], p["top_n"], p["top_text"], p["top_score"], p["res"] + 8,
                                                        p["res"] + 16, p["res"] + 24, p["tmp"], tb, st),
                   f._text(), dict(kept_outs, res=(4, torch.int64), **top_outs), tb,
                   cut=lambda x: kept_cut(x, x["res"][0]) + top_cut(x) + [x["res"]], want=kept_want + top_want + [None])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_score_entry_points_on_a_side_stream(torch_cuda, gates, features, entry):
    bad = sc.exercise(torch_cuda, gates, _case(torch_cuda, features, entry), control=entry == "acm_gpu_score_device")
    assert not bad, "\n".join(bad)
