"""acm_tally without a GPU: a machine with a comparator of its own over 3-byte symbols takes the
caller loop on the host (ACM_SCAN_PATH_CPU_LOOP) and counts there.  The expected answer is
np.bincount over the ORACLE's records (tests/tally_cases.py; the oracle sees the same words over
bytes, the mapping of letters is one to one)."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from tests.batch_cases import KEYWORDS, TEXTS
from tests.tally_cases import PATH_LOOP, byte_oracle, loop_machine, nontrivial, novel_words, oracle_tally, prefilled, sym3

E_ARG = binding.ACM_GPU_E_ARG


def _tally(h, text3, counters, n_keywords=None, with_total=True):
    L = acm.lib()
    t = np.frombuffer(text3, np.uint8).copy() if len(text3) else np.zeros(3, np.uint8)
    total = C.c_uint64(0xDEAD)
    rc = L.acm_tally(h, t.ctypes.data, len(text3) // 3, counters.ctypes.data if counters is not None else None,
                     counters.size if n_keywords is None else n_keywords, C.byref(total) if with_total else None)
    return rc, int(total.value)


def _added_to_and_doubled(h, text, want, n_records):
    """pre-filled counters come back as pattern + bincount, a second call doubles the increment, two
    entries more than the machine has keywords are allowed and stay as they were"""
    L = acm.lib()
    K = want.size
    counters = prefilled(K + 2)
    rc, total = _tally(h, sym3(text), counters)
    assert rc == 0 and L.acm_scan_path(h) == PATH_LOOP
    assert total == n_records == int(want.sum())
    assert np.array_equal(counters[:K], prefilled(K) + want) and np.array_equal(counters[K:], prefilled(K + 2)[K:])
    rc, total = _tally(h, sym3(text), counters)
    assert rc == 0 and total == n_records
    assert np.array_equal(counters[:K], prefilled(K) + 2 * want) and np.array_equal(counters[K:], prefilled(K + 2)[K:])
    # `total` is optional
    zeroed = np.zeros(K, np.uint64)
    assert _tally(h, sym3(text), zeroed, with_total=False)[0] == 0 and np.array_equal(zeroed, want)


def test_nested_suffix_dictionary_on_the_host_loop():
    keywords = KEYWORDS + [b"absent"]
    text = b"".join(TEXTS)
    want, n_records = oracle_tally(byte_oracle(keywords), text)
    nontrivial(want)
    h, keep = loop_machine(keywords)
    assert acm.lib().acm_scan_path(h) == 0
    _added_to_and_doubled(h, text, want, n_records)
    # no text: nothing is added, the total is 0
    counters = prefilled(want.size)
    assert _tally(h, b"", counters) == (0, 0) and np.array_equal(counters, prefilled(want.size))
    acm.lib().acm_release(h)


def test_the_novel_and_a_dictionary_of_its_own_words(novel_bytes):
    keywords = novel_words(novel_bytes)
    text = novel_bytes[:150000]
    want, n_records = oracle_tally(byte_oracle(keywords), text)
    nontrivial(want)
    assert n_records > 10000
    h, keep = loop_machine(keywords)
    _added_to_and_doubled(h, text, want, n_records)
    acm.lib().acm_release(h)


def test_tally_arguments_are_checked_without_a_gpu():
    L = acm.lib()
    h, keep = loop_machine(KEYWORDS)
    text3 = sym3(b"".join(TEXTS))
    counters = prefilled(len(KEYWORDS))
    assert _tally(h, text3, counters, n_keywords=len(KEYWORDS) - 1)[0] == E_ARG       # fewer counters than keywords
    assert _tally(h, text3, counters, n_keywords=0)[0] == E_ARG
    assert _tally(h, text3, None, n_keywords=len(KEYWORDS))[0] == E_ARG               # no counters
    assert _tally(None, text3, counters)[0] == E_ARG                                  # no machine
    t = np.zeros(3, np.uint8)
    assert L.acm_tally(h, None, 5, counters.ctypes.data, counters.size, None) == E_ARG    # symbols, but no text
    assert np.array_equal(counters, prefilled(len(KEYWORDS))) and L.acm_scan_path(h) == 0  # nothing was counted, nothing ran
    assert L.acm_tally(h, t.ctypes.data, 0, counters.ctypes.data, counters.size, None) == 0
    # the plan-level calls refuse the same before they touch a device (there is no plan here: NULL is refused too)
    n = C.c_uint64(0)
    assert L.acm_gpu_tally_host(None, t.ctypes.data, 1, counters.ctypes.data, counters.size, C.byref(n)) == E_ARG
    assert L.acm_gpu_tally_device(None, None, 0, 0, None, 0, 16, 16, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_tally_tmp_bytes(None, 16, 16) == 0
    assert L.acm_gpu_tally_form(None) == E_ARG and L.acm_gpu_tally_keywords(None) == 0
    L.acm_release(h)


def test_library_exports_the_tally_symbols():
    L = acm.lib()
    names = ("acm_gpu_tally_tmp_bytes", "acm_gpu_tally_device", "acm_gpu_tally_host", "acm_tally", "acm_gpu_tally_form", "acm_gpu_tally_keywords")
    for name in names:
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
