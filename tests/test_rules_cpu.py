"""Keyword rules per text without a GPU: acm_rules_check, acm_rules_matrix (the sequential evaluation of
a count matrix) and acm_rules on a machine that takes the caller loop on the host
(ACM_SCAN_PATH_CPU_LOOP).  The expected answer is always the brute-force evaluation, in numpy, of the
ORACLE's count matrix (tests/rules_cases.py)."""
import ctypes as C

import numpy as np

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import absent, between, present, rule
from tests.batch_cases import offsets_of
from tests.grep_cases import GREP_TEXTS
from tests.rules_cases import ALWAYS, M_OF_N, NEVER_RULE, NO_MAX, RULE_KEYWORDS, SHAPES, check, expected_fired, nontrivial
from tests.tally_batch_cases import expected
from tests.tally_cases import PATH_LOOP, byte_oracle, sym3

E_ARG, E_OVERFLOW = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW
GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
K = len(RULE_KEYWORDS)


def _case():
    """(count matrix of the oracle as a TalliedBatch, the rule set, the expected result) of the boundary set"""
    o = byte_oracle(RULE_KEYWORDS)
    text = np.frombuffer(b"".join(GREP_TEXTS), np.uint8)
    counts = expected(o, text, offsets_of(GREP_TEXTS))
    rs = binding.RuleSet(SHAPES)
    nontrivial(GREP_TEXTS, counts, K, rs, m_of_n=M_OF_N, always=ALWAYS, never=(NEVER_RULE,), on_top=GREP_TEXTS.index(b"on top"))
    tallied = binding.TalliedBatch(counts[0], counts[1], counts[2], counts[1].size, int(counts[2].sum()))
    return tallied, rs, expected_fired(counts, K, rs)


def _check_rc(rules, n_keywords=K):
    rs = binding.RuleSet(rules)
    return acm.lib().acm_rules_check(*rs.args(), n_keywords)


def test_rules_check_refuses_every_listed_case():
    assert _check_rc(SHAPES) == 0
    assert _check_rc([]) == 0
    assert _check_rc([rule([between(0, 3, 2)])]) == E_ARG                    # lo > hi
    assert _check_rc([rule([present(0)], 0)]) == E_ARG                       # need = 0
    assert _check_rc([rule([present(0), present(1)], 3)]) == E_ARG           # need above the number of terms
    assert _check_rc([rule([present(K)])]) == E_ARG                          # a keyword id that is none
    assert _check_rc([rule([present(K - 1)])]) == 0
    assert _check_rc([rule([between(0, 0, NO_MAX)])]) == 0                   # always holds: allowed
    L = acm.lib()
    terms = np.array([[0, 1, NO_MAX], [1, 1, NO_MAX]], np.uint32)
    need = np.array([1, 1], np.uint32)

    def call(rule_ptr, n_rules=2, t=terms, nd=need):
        rp = np.array(rule_ptr, np.uint64)
        return L.acm_rules_check(t.ctypes.data if t is not None else None, rp.ctypes.data, nd.ctypes.data if nd is not None else None, n_rules, K)
    assert call([0, 1, 2]) == 0
    assert call([0, 1, 1]) == E_ARG and call([0, 0, 2]) == E_ARG             # a rule without terms
    assert call([0, 2, 1]) == E_ARG                                          # decreasing
    assert call([1, 1, 2]) == E_ARG                                          # does not begin with 0
    assert call([0, 1, 2], n_rules=1 << 31) == E_ARG
    assert call([0, 1, 2], t=None) == E_ARG and call([0, 1, 2], nd=None) == E_ARG
    assert L.acm_rules_check(terms.ctypes.data, None, need.ctypes.data, 2, K) == E_ARG


def test_matrix_on_the_boundary_set():
    tallied, rs, want = _case()
    got = binding.rules_matrix(tallied, rs, K)
    check(got, want, "acm_rules_matrix")
    assert got.rule_hits(rs.n_rules).tolist() == want[2].sum(axis=0).tolist()
    assert np.array_equal(got.to_sparse_csr(rs.n_rules).to_dense().numpy() != 0, want[2])


def _raw(tallied, rs, fired_ptr, fired, cap, n, n_keywords=K, row_ptr=None, col=None):
    rp = tallied.row_ptr if row_ptr is None else row_ptr
    cl = tallied.col if col is None else col
    return acm.lib().acm_rules_matrix(rp.ctypes.data, cl.ctypes.data, tallied.val.ctypes.data, rp.size - 1, n_keywords, *rs.args(),
                                      fired_ptr.ctypes.data if fired_ptr is not None else None, fired.ctypes.data if fired is not None else None,
                                      cap, C.byref(n) if n is not None else None)


def test_matrix_count_only_overflow_by_one_and_guards():
    tallied, rs, want = _case()
    n_texts, k = want[0].size - 1, want[1].size
    n = C.c_uint64(99)
    fired_ptr = np.full(n_texts + 1, GUARD64, np.uint64)
    assert _raw(tallied, rs, fired_ptr, None, 0, n) == 0                     # `fired` NULL: the call only counts
    assert n.value == k and np.array_equal(fired_ptr, want[0])
    fired = np.full(k - 1, GUARD32, np.uint32)
    fired_ptr[:] = GUARD64
    n.value = 99
    assert _raw(tallied, rs, fired_ptr, fired, k - 1, n) == E_OVERFLOW
    assert n.value == k and np.all(fired == GUARD32) and np.array_equal(fired_ptr, want[0])
    fired = np.full(k + 3, GUARD32, np.uint32)
    assert _raw(tallied, rs, fired_ptr, fired, k, n) == 0
    assert np.array_equal(fired[:k], want[1]) and np.all(fired[k:] == GUARD32)


def test_matrix_arguments_and_no_text():
    tallied, rs, want = _case()
    n_texts = want[0].size - 1
    n = C.c_uint64(0)
    fired_ptr, fired = np.zeros(n_texts + 1, np.uint64), np.zeros(want[1].size, np.uint32)
    assert _raw(tallied, rs, fired_ptr, fired, fired.size, n) == 0
    down = tallied.row_ptr.copy()
    down[3], down[4] = tallied.row_ptr[4] + 1, tallied.row_ptr[3]
    assert down[3] > down[4] and _raw(tallied, rs, fired_ptr, fired, fired.size, n, row_ptr=down) == E_ARG
    one = tallied.row_ptr.copy()
    one[0] = 1
    assert _raw(tallied, rs, fired_ptr, fired, fired.size, n, row_ptr=one) == E_ARG
    high = tallied.col.copy()
    high[0] = K
    assert _raw(tallied, rs, fired_ptr, fired, fired.size, n, col=high) == E_ARG             # a col >= n_keywords
    assert _raw(tallied, rs, None, fired, fired.size, n) == E_ARG and _raw(tallied, rs, fired_ptr, fired, fired.size, None) == E_ARG
    assert _raw(tallied, binding.RuleSet([rule([present(0)], 2)]), fired_ptr, fired, fired.size, n) == E_ARG
    # no text at all: fired_ptr[0] = 0, nothing fired -- not even the always-rule
    empty = binding.TalliedBatch(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0, 0)
    got = binding.rules_matrix(empty, rs, K)
    assert got.n_fired == 0 and got.fired_ptr.tolist() == [0] and got.fired.size == 0
    # texts without any keyword: the two rules that fire by their base (he absent; the cancelling rule), in every one of them
    got = binding.rules_matrix(binding.TalliedBatch(np.zeros(4, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0, 0), rs, K)
    assert got.fired_ptr.tolist() == [0, 2, 4, 6] and got.fired.tolist() == [ALWAYS, 7] * 3


def test_matrix_a_count_above_two_to_the_32():
    rs = binding.RuleSet([rule([present(1)]), rule([between(1, 1, 0xFFFFFFFE)]), rule([absent(1)])])
    big = binding.TalliedBatch(np.array([0, 1, 1], np.uint64), np.array([1], np.uint32), np.array([(1 << 32) + 5], np.uint64), 1, (1 << 32) + 5)
    got = binding.rules_matrix(big, rs, 2)
    assert got.fired_ptr.tolist() == [0, 1, 2] and got.fired.tolist() == [0, 2]     # no upper bound holds, an upper bound of 2^32 - 2 does not


def test_machine_rules_on_the_host_loop():
    """3-byte symbols: no GPU path takes the machine.  "us|hers" and "sh|e" cut a keyword by a text boundary"""
    tallied, rs, want = _case()
    m = acm.Machine(3)                                                   # ACM_CMP_DEFAULT over 3 bytes: the host loop
    for kw in RULE_KEYWORDS:
        buf = np.frombuffer(sym3(kw), np.uint8).copy()
        m._keep.append(buf)
        cur = C.c_void_p(m.L.acm_initiate(m.handle))
        for i in range(len(kw)):
            m.L.acm_insert_letter_of_keyword(C.byref(cur), buf.ctypes.data + 3 * i)
        m.L.acm_insert_end_of_keyword(C.byref(cur), None, None)
    got = m.rules([sym3(t) for t in GREP_TEXTS], rs)
    assert m.scan_path == PATH_LOOP
    check(got, want, "Machine.rules")
    assert got.total == tallied.total
    # through the C call: one entry too little room is an overflow that leaves `fired` alone; the path is recorded
    raw = np.frombuffer(b"".join(sym3(t) for t in GREP_TEXTS), np.uint8).copy()
    off = offsets_of(GREP_TEXTS)
    k = want[1].size
    fired_ptr, fired = np.zeros(off.size, np.uint64), np.full(k - 1, GUARD32, np.uint32)
    n, total = C.c_uint64(99), C.c_uint64(99)
    rc = m.L.acm_rules(m.handle, raw.ctypes.data, off.ctypes.data, off.size - 1, *rs.args(), fired_ptr.ctypes.data, fired.ctypes.data, k - 1,
                       C.byref(n), C.byref(total))
    assert rc == E_OVERFLOW and n.value == k and total.value == tallied.total and np.array_equal(fired_ptr, want[0]) and np.all(fired == GUARD32)
    assert m.rules([], rs).fired_ptr.tolist() == [0]
    bad = binding.RuleSet([rule([present(K)])])
    assert m.L.acm_rules(m.handle, raw.ctypes.data, off.ctypes.data, off.size - 1, *bad.args(), fired_ptr.ctypes.data, None, 0, C.byref(n), None) == E_ARG


def test_plan_level_calls_refuse_before_they_touch_a_device():
    L = acm.lib()
    n = C.c_uint64(0)
    off = np.zeros(1, np.uint64)
    rs = binding.RuleSet(SHAPES)
    h = C.c_void_p()
    assert L.acm_gpu_rules_create(None, *rs.args(), C.byref(h)) == E_ARG
    assert L.acm_gpu_rules_matrix_tmp_bytes(None, None, 0) == 0 and L.acm_gpu_rules_tmp_bytes(None, None, 16, 16, 16, 0, 0) == 0
    assert L.acm_gpu_rules_matrix_device(None, None, None, None, None, 0, None, None, 0, None, None, 0, None) == E_ARG
    assert L.acm_gpu_rules_device(None, None, None, 0, None, 0, 16, 16, 16, None, None, 0, None, None, None, None, None, 0, None) == E_ARG
    assert L.acm_gpu_rules_host(None, None, off.ctypes.data, 0, *rs.args(), off.ctypes.data, None, 0, C.byref(n), None) == E_ARG
    assert L.acm_gpu_rules_info(None, None) == E_ARG
    L.acm_gpu_rules_destroy(None)


def test_library_exports_the_rules_symbols():
    L = acm.lib()
    for name in ("acm_rules_check", "acm_rules_matrix", "acm_gpu_rules_create", "acm_gpu_rules_destroy", "acm_gpu_rules_info",
                 "acm_gpu_rules_matrix_tmp_bytes", "acm_gpu_rules_matrix_device", "acm_gpu_rules_tmp_bytes", "acm_gpu_rules_device",
                 "acm_gpu_rules_host", "acm_rules"):
        assert name in binding.EXPORTS and getattr(L, name) is not None, name
