"""The two device entry points of include/acm_segment.h on a stream that is not the default one: the EARLY / LATE /
CONTROL arrangements of tests/stream_cases.py (Gates, Case, exercise), over the dense batch of tests/test_streams_gpu.py.
The expected value is the plain call's on the null stream, held here against the definition of SEGMENT over the
oracle's records as well."""
import os

import numpy as np
import pytest

from aho_corasick_1975_amd import binding
from tests import stream_cases as sc
from tests.cases import build_pair
from tests.segment_cases import define
from tests.test_scratch_bounds_gpu import KEYWORDS, _batch
from tests.test_streams_gpu import _decoy_batch

HEADER = os.path.join(sc.ROOT, "include", "acm_segment.h")
ENTRIES = ["acm_gpu_segment_records_device", "acm_gpu_scan_segment_device"]
GAP = 3


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


def _costs(f):
    return (2 + np.arange(f.K) % 4).astype(np.uint32)


def _case(torch, f, name):
    L, h, N, CAP = binding.lib(), f.plan.h, f.N, sc.CAP
    cost = _costs(f)
    d_cost = sc.dev(torch, cost)
    outs = {"count": (1, torch.int64), "sums": (2, torch.int64)}
    if name == "acm_gpu_segment_records_device":
        tb = L.acm_gpu_segment_tmp_bytes(h, CAP, N)
        gated, n = f._records()
        del gated["text"]
        want = define(f.rec[:n], cost, GAP)[0]
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_segment_records_device(h, p["rec"], CAP, p["n"], 0, N, d_cost.data_ptr(), cost.size, GAP, p["out"],
                                                                      p["count"], p["sums"], p["tmp"], tb, st),
                       gated, dict(outs, out=(2 * CAP, torch.int64)), tb,
                       cut=lambda x: [sc.rows(x, "out", x["count"][0]), x["count"], x["sums"]], want=[sc.rec_rows(want), None, None], keep=(d_cost,))
    tb = L.acm_gpu_scan_segment_tmp_bytes(h, CAP, N, 0)
    want = define(f.o.scan(f.real), cost, GAP)[0]
    return sc.Case(name, f.plan,
                   lambda p, st: L.acm_gpu_scan_segment_device(h, p["text"], N, 0, None, 0, d_cost.data_ptr(), cost.size, GAP, p["rec"], CAP,
                                                               p["count"], p["sums"], p["tmp"], tb, st),
                   f._text(), dict(outs, rec=(2 * CAP, torch.int64)), tb,
                   cut=lambda x: [sc.rows(x, "rec", x["count"][0]), x["count"], x["sums"]], want=[sc.rec_rows(want), None, None], keep=(d_cost,))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_segment_entry_points_on_a_side_stream(torch_cuda, gates, features, entry):
    bad = sc.exercise(torch_cuda, gates, _case(torch_cuda, features, entry), control=entry == "acm_gpu_scan_segment_device")
    assert not bad, "\n".join(bad)
