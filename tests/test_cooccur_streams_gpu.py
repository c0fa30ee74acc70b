"""The three device entry points of include/acm_cooccur.h on a stream that is not the default one: the EARLY / LATE /
CONTROL arrangements of tests/stream_cases.py (Gates, Case, exercise), over the dense batch of tests/test_streams_gpu.py.
The matrix call and the fused call run with flags 0 (the radix sort of the keys alone) and under PRODUCT (the sort of pairs
and the running sum of the weights), ADD always sorts pairs: the memset of the scratch head, the three scans, either sort
and the tally in front all have to be queued on the caller's stream.  The expected value is the plain call's on the null
stream, held here against the brute force of the definition over the oracle's count matrix as well (the cases:
tests/cooccur_stream_cases.py).  A call without a text (the memsets of the empty result) is held to the same."""
import os

import numpy as np
import pytest

from aho_corasick_1975_amd import binding
from tests import cooccur_stream_cases as cc
from tests import stream_cases as sc
from tests.cases import build_pair
from tests.test_scratch_bounds_gpu import KEYWORDS, _batch
from tests.test_streams_gpu import _decoy_batch

HEADER = os.path.join(sc.ROOT, "include", "acm_cooccur.h")
ENTRIES = cc.ENTRIES


def test_every_stream_entry_point_of_the_header_is_exercised():
    assert sorted(sc.header_stream_functions(path=HEADER)) == sorted(ENTRIES) == sorted(set(name for name, _ in cc.CASES))


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


@pytest.mark.gpu
@pytest.mark.parametrize("entry,flags", cc.CASES)
def test_cooccur_entry_points_on_a_side_stream(torch_cuda, gates, features, entry, flags):
    bad = sc.exercise(torch_cuda, gates, cc.case(torch_cuda, features, entry, flags), control=entry == "acm_gpu_cooccur_device" and flags == 0)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_the_empty_result_is_set_on_the_callers_stream(torch_cuda, gates, features):
    """n_texts = 0: co_ptr, nnz, cross and skipped are set by memsets; behind a gate on the side stream they are still
    what the caller left there when the call returns, and zero once the stream has passed"""
    torch, L, K = torch_cuda, binding.lib(), features.K
    for fused in (False, True):
        out = torch.full((K + 1 + 6,), 0x5A, dtype=torch.int64, device="cuda")
        zero = torch.zeros(1, dtype=torch.int64, device="cuda")
        p = out.data_ptr()
        res = p + 8 * (K + 1)
        tb = L.acm_gpu_cooccur_tmp_bytes(features.plan.h, sc.WINDOW, sc.CAP, sc.CAP, 0, 0, K, 8) if fused else 0
        tmp = torch.zeros(max(tb, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(gates.side):
            gates.sleep(100.0)
            if fused:
                rc = L.acm_gpu_cooccur_device(features.plan.h, zero.data_ptr(), 0, zero.data_ptr(), 0, sc.WINDOW, sc.CAP, sc.CAP, K, 0, 0, 8, p, None, None, 0, res,
                                              res + 8, res + 16, res + 24, res + 32, res + 40, tmp.data_ptr(), tb, gates.side.cuda_stream)
            else:
                rc = L.acm_gpu_cooccur_matrix_device(features.plan.h, zero.data_ptr(), None, None, 0, K, 0, 0, 8, p, None, None, 0, res, res + 8, res + 16,
                                                     None, 0, gates.side.cuda_stream)
            asynchronous = not gates.side.query()
        snap = out.clone()                                   # on the null stream, which the gate does not hold up
        torch.cuda.default_stream().synchronize()
        still_gated = not gates.side.query()
        assert rc == 0 and asynchronous and still_gated, (fused, rc, asynchronous, still_gated)
        assert bool((snap == 0x5A).all()), (fused, "something was written in front of the gate", snap.cpu().tolist())
        gates.side.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[:K + 1 + 3] == 0), (fused, got)
        features.plan.status()
