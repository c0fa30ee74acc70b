"""The inputs of test_long_keywords_gpu.py, checked from the CPU oracle alone (a GPU failure there is
then the kernel's, not the case's), and the flattened tables and the oracle against each other at
keyword lengths on either side of the lmax thresholds."""
import numpy as np
import pytest

from tests import long_cases as lc
from tests.brute import brute_records
from tests.flatwalk import walk_csr, walk_dense


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_has_what_the_gpu_tests_rely_on(name):
    p = lc.params(name)
    n, lmax = p["n"], p["lmax"]
    kws, text = lc.case(name)
    assert text.size == n and max(w.size for w in kws) == lmax == kws[0].size == kws[1].size
    if not p.get("shorts", True):
        assert min(w.size for w in kws) >= 4
    o, want = lc.answer(name)
    assert o.lmax == lmax
    full = want[want["length"] == lmax]
    print("%s: %d records, %d of full length" % (name, want.size, full.size))
    assert full.size >= 100
    assert (full["end_pos"] == lmax - 1).any() and (full["end_pos"] == n - 1).any()
    _, per_pos = np.unique(want["end_pos"], return_counts=True)
    assert per_pos.max() >= 4
    # the near miss: S without its last symbol, then a symbol outside the alphabet
    assert not (full["end_pos"] == n // 2 + lmax - 1).any()
    assert (want["end_pos"] == n // 2 + lmax - 2).any()        # ... but its prefix of lmax - 1 symbols is a keyword
    # S across a multiple of every boundary size, and the periodic keyword at every second position of its run
    ends = lc.spine_ends(name)
    for b in (b for b in lc.boundary_sizes(lmax) if b < n):
        assert ((ends // b) != ((ends - lmax + 1) // b)).any(), b
        assert (ends % b == 0).any(), ("no S with only its last symbol behind a multiple of", b)
        assert ((ends - lmax + 1) % b == b - 1).any(), ("no S with only its first symbol before a multiple of", b)
    run_end = n // 3 + lmax + lc.RUN_EXTRA
    p_ends = want["end_pos"][(want["keyword_id"] == 1) & (want["length"] == lmax)].astype(np.int64)
    assert np.array_equal(p_ends[(p_ends >= n // 3) & (p_ends < run_end)], np.arange(n // 3 + lmax - 1, run_end, 2))


@pytest.mark.parametrize("name,seg_log2", lc.SEAM_CASES)
def test_spine_lies_across_launch_segment_seams(name, seg_log2):
    lmax = lc.params(name)["lmax"]
    assert lc.seams_crossed(name, seg_log2).max() >= (2 if lmax > (1 << seg_log2) else 1)
    assert (lc.spine_ends(name) % (1 << seg_log2) == 0).any()
    assert lc.params(name)["n"] >> seg_log2 >= 4


def test_spine_lies_across_shard_cuts():
    for name in ("dense-1025", "gram2-1025", "starts32-1025", "csr-4082"):
        n, lmax = lc.params(name)["n"], lc.params(name)["lmax"]
        ends = lc.spine_ends(name)
        cuts = np.array([n * r // 4 for r in range(1, 4)])
        assert ((ends[:, None] >= cuts) & (ends[:, None] - lmax + 1 < cuts)).any()
        assert np.isin(ends, cuts).any()


def test_sticky_cases_have_more_states_than_two_byte_entries_address():
    for name in ("sticky-256", "sticky-4081"):
        assert lc.machine(name).flatten().info.n_states > 32768
    for name in ("dense-4081", "gram2-4081"):
        assert lc.machine(name).flatten().info.n_states <= 32768


@pytest.mark.parametrize("name", ["dense-65", "dense-1025", "csr-4082", "starts32-1025"])
def test_flattened_tables_walked_on_the_cpu_equal_the_oracle(name):
    kws, text = lc.case(name)
    _, want = lc.answer(name)
    flat = lc.machine(name).flatten()
    assert flat.info.lmax == lc.params(name)["lmax"]
    assert np.array_equal(walk_csr(flat, text), want)
    if name.startswith("dense"):
        assert np.array_equal(walk_dense(flat, text), want)
    cut = int(lc.spine_ends(name)[1]) - 3       # inside a planted S: it is reported, with a far pos_base too
    o = lc.answer(name)[0]
    assert np.array_equal(walk_csr(flat, text, emit_from=cut, pos_base=1 << 40), o.scan(text, pos_base=1 << 40, emit_from=cut))


def test_brute_force_equals_the_oracle_on_a_miniature():
    kws, text = lc.long_case(seed=5, sym=1, lmax=65, n_long=4, n=3000, lo=97, span=4)
    o = lc.po.Oracle(1, lc.po.AC75)
    for w in kws:
        o.add_keyword(w)
    want = o.scan(text)
    assert (want["length"] == 65).sum() >= 100
    assert np.array_equal(brute_records([w.tolist() for w in kws], text.tolist()), want)
