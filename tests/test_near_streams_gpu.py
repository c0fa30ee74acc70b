"""The two device entry points of include/acm_near.h on a stream that is not the default one: the EARLY / LATE /
CONTROL arrangements of tests/stream_cases.py (Gates, Case, exercise), over the dense batch of tests/test_streams_gpu.py.
The expected value is the plain call's on the null stream, held here against the definition of NEAR over the
oracle's records (tests/near_cases.py) as well (the cases: tests/family_stream_cases.py)."""
import os

import pytest

from tests import family_stream_cases as fc
from tests import stream_cases as sc
from tests.cases import build_pair
from tests.test_scratch_bounds_gpu import KEYWORDS, _batch
from tests.test_streams_gpu import _decoy_batch

HEADER = os.path.join(sc.ROOT, "include", "acm_near.h")
ENTRIES = fc.NEAR


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


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_near_entry_points_on_a_side_stream(torch_cuda, gates, features, entry):
    bad = sc.exercise(torch_cuda, gates, fc.near_case(torch_cuda, features, entry), control=entry == "acm_gpu_scan_near_device")
    assert not bad, "\n".join(bad)
