"""The two device entry points of include/acm_near.h on a stream that is not the default one: the EARLY / LATE /
CONTROL arrangements of tests/stream_cases.py (Gates, Case, exercise), over the dense batch of tests/test_streams_gpu.py.
The expected value is the plain call's on the null stream, held here against the definition of NEAR over the
oracle's records (tests/near_cases.py) as well."""
import os

import numpy as np
import pytest

from aho_corasick_1975_amd import binding
from tests import stream_cases as sc
from tests.cases import build_pair
from tests.near_cases import near
from tests.test_scratch_bounds_gpu import KEYWORDS, _batch
from tests.test_streams_gpu import _decoy_batch

HEADER = os.path.join(sc.ROOT, "include", "acm_near.h")
ENTRIES = ["acm_gpu_near_records_device", "acm_gpu_scan_near_device"]


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
    f = sc.Features(torch_cuda, m, o, m.plan, text, _decoy_batch(), off)
    # the groups: the two keywords the batch holds most often (the chain set's) near each other, and either of them
    a, b = (int(x) for x in f.chainset.terms[:2, 0])
    f.near_groups = [([a, b], 40, 0), ([b, a], 25, 1)]
    f.handles["near"] = f.plan.near(f.near_groups)
    return f


def _case(f, name):
    most = int(f.handle("near").info()["max_postings"])
    if name == "acm_gpu_near_records_device":
        case = f._join_records(name, "near", most)
        want = near(f.rec[:f.n], f.near_groups, f.N, f.off)
    else:
        case = f._join_scan(name, "near", most)
        want = near(f.o.scan(f.real), f.near_groups, f.N, f.off)
    assert want.size >= 16
    case.want = [sc.rec_rows(want), None]
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_near_entry_points_on_a_side_stream(torch_cuda, gates, features, entry):
    bad = sc.exercise(torch_cuda, gates, _case(features, entry), control=entry == "acm_gpu_scan_near_device")
    assert not bad, "\n".join(bad)
