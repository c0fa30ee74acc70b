"""Shared by the rules tests (test_rules_cpu.py, test_rules_gpu.py): the rule-shape set over the
boundary keywords, the expected text x rule matrix -- always the brute-force evaluation, in numpy, of
the ORACLE's count matrix (tests/tally_batch_cases.expected and dense), never of the library's own
counts --, the check of a result against it and the check that a workload cannot pass trivially."""
import numpy as np

from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import absent, between, present, rule
from tests.batch_cases import KEYWORDS
from tests.tally_batch_cases import dense

NO_MAX = binding.ACM_RULE_NO_MAX
HE, SHE, HERS, S = 0, 1, 2, 3
assert [KEYWORDS[k] for k in (HE, SHE, HERS, S)] == [b"he", b"she", b"hers", b"s"]
# the boundary keywords and one more that no text of the boundary set holds (keyword ids are insertion ranks:
# the first four stay what they are)
NEVER = len(KEYWORDS)
RULE_KEYWORDS = KEYWORDS + [b"qux"]

SHAPES = [
    rule([present(HE), present(HERS)]),                                      # 0  AND
    rule([present(SHE), present(HERS)], 1),                                  # 1  OR
    rule([present(S), absent(HE)]),                                          # 2  s present and he absent
    rule([present(HE), present(SHE), present(HERS), present(S, 2)], 2),      # 3  2 of 4
    rule([absent(HE)]),                                                      # 4  an always-rule
    rule([between(S, 2, 3)]),                                                # 5  an interval
    rule([between(HE, 1, 1), present(HE, 4)], 1),                            # 6  one keyword twice
    rule([absent(HE), present(S)], 1),                                       # 7  cancelling: on "hers" -1 + 1, fires by its base (an always-rule too); not on "xhe"
    rule([between(SHE, 0, NO_MAX), present(HERS)]),                          # 8  a term that holds at every count
    rule([present(NEVER)]),                                                  # 9  a keyword that occurs in no text
]
M_OF_N, ALWAYS, NEVER_RULE = 3, 4, 9


def holding(want, n_keywords, ruleset):
    """held[t][r] = how many terms of rule r hold for text t, from the dense matrix"""
    rs = ruleset if isinstance(ruleset, binding.RuleSet) else binding.RuleSet(ruleset)
    counts = dense(want, n_keywords)
    held = np.zeros((counts.shape[0], rs.n_rules), np.int64)
    for r in range(rs.n_rules):
        for k, lo, hi in rs.terms[int(rs.rule_ptr[r]):int(rs.rule_ptr[r + 1])].tolist():
            c = counts[:, k]
            held[:, r] += (c >= lo) & ((c <= hi) if hi != NO_MAX else True)
    return held, rs


def expected_fired(want, n_keywords, ruleset):
    """(fired_ptr, fired, the boolean matrix) of the oracle's count matrix `want` = (row_ptr, col, val): the brute force"""
    held, rs = holding(want, n_keywords, ruleset)
    fires = held >= rs.need.astype(np.int64)[None, :]
    fired_ptr = np.concatenate([[0], np.cumsum(fires.sum(axis=1))]).astype(np.uint64)
    return fired_ptr, np.nonzero(fires)[1].astype(np.uint32), fires


def check(got, want, what=""):
    """a Fired of numpy arrays cut to size against (fired_ptr, fired, ...)"""
    fired_ptr, fired = want[0], want[1]
    assert got.n_fired == fired.size, (what, "n_fired", got.n_fired, fired.size)
    assert np.array_equal(np.asarray(got.fired_ptr).astype(np.uint64), fired_ptr), (what, "fired_ptr")
    assert np.array_equal(np.asarray(got.fired).astype(np.uint32), fired), (what, "fired")
    for t in range(fired_ptr.size - 1):                                    # (implied by the equality above; said on its own)
        row = np.asarray(got.fired[int(fired_ptr[t]):int(fired_ptr[t + 1])]).astype(np.int64)
        assert np.all(np.diff(row) > 0), (what, "row not ascending", t)


def nontrivial(texts, want, n_keywords, ruleset, m_of_n=None, always=None, never=(), on_top=None):
    """from the oracle alone: every rule but those of `never` fires somewhere, every rule leaves a text
    out, a row fires two rules or more; the always-rule fires on an empty text and on the non-empty
    text `on_top`; the m-of-n rule has a text with exactly need and one with exactly need - 1 holding
    terms; a non-empty text fires no rule -- or the assert says which rules forbid that"""
    held, rs = holding(want, n_keywords, ruleset)
    fires = held >= rs.need.astype(np.int64)[None, :]
    lens = np.array([len(t) for t in texts])
    per_rule, per_text = fires.sum(axis=0), fires.sum(axis=1)
    print("texts %d, rules %d, fired %d, per rule %s, widest row %d" % (lens.size, rs.n_rules, int(fires.sum()), per_rule.tolist(), int(per_text.max())))
    for r in range(rs.n_rules):
        assert (per_rule[r] == 0) == (r in never), ("fires nowhere", r)
        assert per_rule[r] < lens.size, ("fires everywhere", r)
    assert np.any(per_text >= 2)
    if always is not None:
        assert np.any(fires[lens == 0, always]) and fires[on_top, always] and lens[on_top] > 0
    if m_of_n is not None:
        need = int(rs.need[m_of_n])
        assert np.any(held[:, m_of_n] == need) and np.any(held[:, m_of_n] == need - 1)
    base = np.array([int(np.count_nonzero(rs.terms[int(rs.rule_ptr[r]):int(rs.rule_ptr[r + 1]), 1] == 0)) for r in range(rs.n_rules)])
    always_rules = np.flatnonzero(base >= rs.need.astype(np.int64))         # they fire on a row without any keyword
    silent = (per_text == 0) & (lens > 0)
    if not np.any(silent):
        others = sorted(set(np.nonzero(fires[lens > 0])[1].tolist()) - set(always_rules.tolist()))
        assert always_rules.size > 0, "every non-empty text fires a rule although no rule fires on an empty row"
        print("no non-empty text without a rule: the always-rules %s fire wherever their keywords are missing, and every text that holds those "
              "fires one of %s" % (always_rules.tolist(), others))
