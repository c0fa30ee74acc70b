"""Without a GPU: the growth shapes of tests/growth_cases.py cannot pass trivially, and the sweep of
tests/test_growth_gpu.py is complete.  From the oracle, the definitions and flatten ().info alone."""
import os

import numpy as np
import pytest

from tests import family_stream_cases as fc
from tests import growth_cases as gc
from tests import stream_cases as sc

HEADERS = ["acm_gpu.h", "acm_segment.h", "acm_score.h", "acm_index.h", "acm_near.h"]


def test_the_sweep_holds_every_stream_entry_point_of_the_headers():
    """every function the headers declare with a `void *stream` is swept or excluded with a reason, and nothing else is"""
    declared = [f for h in HEADERS for f in sc.header_stream_functions(os.path.join(sc.ROOT, "include", h))]
    assert len(set(declared)) == len(declared) >= 50
    assert len(set(gc.ENTRIES)) == len(gc.ENTRIES) and not set(gc.ENTRIES) & set(gc.EXCLUDED)
    assert sorted(gc.ENTRIES + list(gc.EXCLUDED)) == sorted(declared)
    assert set(gc.ENTRIES) == set(sc.PLAIN + sc.FEATURES + sc.ANCHORED + fc.SEGMENT + fc.SCORE + fc.INDEX + fc.NEAR)
    assert all(isinstance(r, str) and len(r) > 20 for r in gc.EXCLUDED.values())


@pytest.fixture(scope="module")
def byte_features():
    return gc.features(None, "built")


@pytest.fixture(scope="module")
def gram_features():
    return gc.features(None, "gram_base")


def _features(shape, byte_features, gram_features):
    return gram_features if shape == "gram_base" else byte_features


@pytest.mark.parametrize("shape", gc.SHAPES)
def test_every_shape_ends_with_the_controls_keywords(shape, byte_features, gram_features):
    """the shadow machine of a shape, filled group by group, holds the final machine's keywords id for id"""
    f = _features(shape, byte_features, gram_features)
    kws = gc.keywords_of(f.m)
    groups = gc.steps(shape, f.K, getattr(f, "base_keywords", None))
    assert [k for g in groups for k in g] == list(range(f.K)) and (shape == "built" or len(groups) >= 2)
    assert all(len(g) > 0 for g in groups[1:])           # (an update without a new keyword returns early)
    got = gc.keywords_of(gc.shadow_of(kws, groups))
    assert len(got) == f.K and all(np.array_equal(a, b) for a, b in zip(got, kws))
    assert f.o.nb_keywords == f.K


def test_the_trailing_keyword_is_no_piece_of_a_set(byte_features):
    f = byte_features
    assert bytes(gc.keywords_of(f.m)[-1]) == gc.TRAILING
    for s in (f.patternset, f.chainset, f.ruleset, f.approxset, f.templateset):
        assert int(np.asarray(s.terms)[:, 0].max()) < f.K - 1
    assert np.count_nonzero(f.whole["real"]["keyword_id"] == f.K - 1) > 0        # and it matches


def test_outgrown_the_delta_exceeds_the_base(byte_features):
    """longest keyword, outputs per state and alphabet: a consumer that reads any of them from the base plan alone is wrong"""
    f = byte_features
    kws = gc.keywords_of(f.m)
    base, delta = gc.steps("outgrown", f.K)
    b = gc.shadow_of(kws, [base]).flatten().info
    d = gc.shadow_of(kws, [delta]).flatten().info
    print("base lmax %d outputs %d alphabet %d+%d; delta lmax %d outputs %d alphabet %d+%d" % (
        b.lmax, b.max_outputs, b.alpha_lo, b.alpha_span, d.lmax, d.max_outputs, d.alpha_lo, d.alpha_span))
    assert d.lmax > b.lmax and d.max_outputs > b.max_outputs
    symbols = {int(x) for k in delta for x in kws[k]}
    assert any(not (b.alpha_lo <= x <= b.alpha_lo + b.alpha_span) for x in symbols)
    # and the delta's keywords do match, with those facts: a record longer than the base's longest keyword
    rec = f.whole["real"]
    assert np.count_nonzero(rec["length"] > b.lmax) > 0 and np.count_nonzero(rec["keyword_id"] >= 1) > rec.size // 2


def test_gram_base_the_sets_add_short_pieces(gram_features):
    f = gram_features
    base = f.base_keywords
    assert f.K > base
    lens = [k.size for k in gc.keywords_of(f.m)[base:]]
    rec = f.whole["real"]
    print("pieces %s, their records %d of %d" % (lens, np.count_nonzero(rec["keyword_id"] >= base), rec.size))
    assert np.count_nonzero(rec["keyword_id"] >= base) > 0 and min(lens) < 4


@pytest.mark.parametrize("kind", ["bytes", "gram"])
def test_every_expected_value_is_there_and_tells_real_from_decoy(kind, byte_features, gram_features):
    """no entry point of the sweep can pass on an empty answer or on the other batch's answer"""
    f = gram_features if kind == "gram" else byte_features
    assert all(isinstance(r, str) and len(r) > 20 for r in sc.PLAIN_BY_PLAN.values()) and set(sc.PLAIN_BY_PLAN) <= set(sc.PLAIN)
    for name in gc.ENTRIES:
        if name in sc.PLAIN_BY_PLAN:
            continue
        real, decoy = gc.expected(f, name, "real"), gc.expected(f, name, "decoy")
        assert real is not None and real[0] is not None and real[0].size > 0 and np.any(real[0] != 0), name
        assert any(r is not None and (r.shape != d.shape or not np.array_equal(r, d)) for r, d in zip(real, decoy)), name
        assert sum(r is None for r in real) <= 1, name   # (at most the one array that holds a scratch diagnostic)
