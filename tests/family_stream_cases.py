"""Shared by tests/test_{segment,score,index,near}_streams_gpu.py and tests/test_growth_gpu.py: a Case
(tests/stream_cases.py) per device entry point of include/acm_segment.h, acm_score.h, acm_index.h and acm_near.h over a
stream_cases.Features, with its expected value -- the family's definition in plain Python (tests/segment_cases.py,
score_cases.py, index_cases.py, near_cases.py) over the oracle's records, never the library's own scan.  expected (f, name,
"real" or "decoy") gives that value without a device or a plan (a Features made with torch None will do)."""
import numpy as np

from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import score_class, weight
from tests import stream_cases as sc
from tests.index_cases import brute_force, concat_expected, cut_rows, forms_of
from tests.near_cases import near
from tests.score_cases import expected_scored
from tests.segment_cases import define

SEGMENT = ["acm_gpu_segment_records_device", "acm_gpu_scan_segment_device"]
SCORE = ["acm_gpu_score_matrix_device", "acm_gpu_score_top_device", "acm_gpu_score_device"]
INDEX = ["acm_gpu_index_matrix_device", "acm_gpu_index_concat_device", "acm_gpu_index_device"]
NEAR = ["acm_gpu_near_records_device", "acm_gpu_scan_near_device"]
ENTRIES = SEGMENT + SCORE + INDEX + NEAR
GAP = 3                                                  # segment: the cost of a symbol no keyword covers
TOP = 4                                                  # score: texts per class
BASE = 1000                                              # index: the id of the batch's first text


def _pad(a, room):
    return np.concatenate([a, np.zeros(room - a.size, a.dtype)])


def _counts(f, rec):
    rp, c, v = f._matrix(rec)
    return rp.astype(np.uint64), c.astype(np.uint32), v.astype(np.uint64)


# ---------------------------------------------------------------------------------------------- segment
def segment_costs(f):
    return (2 + np.arange(f.K) % 4).astype(np.uint32)


def segment_expected(f, name, which="real"):
    """SEGMENT of the batch's first n records, or (the fused form) of the records of the buffer as one text, their number
    and include/acm_segment.h's sums[]: the cost[keyword_id] of the emitted records and their lengths, summed"""
    _, rec, _, whole = f._side(which)
    cost = segment_costs(f)
    want = define(rec[:f.n] if name == "acm_gpu_segment_records_device" else whole, cost, GAP)[0]
    sums = [int(cost[want["keyword_id"]].astype(np.int64).sum()), int(want["length"].astype(np.int64).sum())]
    return [sc.rec_rows(want), np.array([want.size]), np.array(sums)]


def segment_case(torch, f, name):
    L, h, N, CAP = binding.lib(), f.plan.h, f.N, sc.CAP
    cost = segment_costs(f)
    d_cost = sc.dev(torch, cost)
    outs = {"count": (1, torch.int64), "sums": (2, torch.int64)}
    if name == "acm_gpu_segment_records_device":
        tb = L.acm_gpu_segment_tmp_bytes(h, CAP, N)
        gated, n = f._records()
        del gated["text"]
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_segment_records_device(h, p["rec"], CAP, p["n"], 0, N, d_cost.data_ptr(), cost.size, GAP, p["out"],
                                                                      p["count"], p["sums"], p["tmp"], tb, st),
                       gated, dict(outs, out=(2 * CAP, torch.int64)), tb,
                       cut=lambda x: [sc.rows(x, "out", x["count"][0]), x["count"], x["sums"]], want=segment_expected(f, name), keep=(d_cost,))
    tb = L.acm_gpu_scan_segment_tmp_bytes(h, CAP, N, 0)
    return sc.Case(name, f.plan,
                   lambda p, st: L.acm_gpu_scan_segment_device(h, p["text"], N, 0, None, 0, d_cost.data_ptr(), cost.size, GAP, p["rec"], CAP,
                                                               p["count"], p["sums"], p["tmp"], tb, st),
                   f._text(), dict(outs, rec=(2 * CAP, torch.int64)), tb,
                   cut=lambda x: [sc.rows(x, "rec", x["count"][0]), x["count"], x["sums"]], want=segment_expected(f, name), keep=(d_cost,))


# ---------------------------------------------------------------------------------------------- score
def score_model(f):
    """over the two keywords the real batch holds most often (the ones f.ruleset is made of)"""
    a, b = int(f.ruleset.terms[0][0]), int(f.ruleset.terms[1][0])
    return binding.ScoreModel([score_class([weight(a, 3), weight(b, -2)]), score_class([weight(b, 2, 2)], threshold=2),
                               score_class([weight(a, -1)], bias=1), score_class([weight(a, 1), weight(b, 1)], threshold=3)])


def score_handle(f):
    """the model compiled on f.plan as it is now, once"""
    if "score" not in f.handles:
        f.handles["score"] = f.plan.score_create(score_model(f))
    return f.handles["score"]


def _scored(f, rec, sm):
    return expected_scored(_counts(f, rec), sm)


def score_expected(f, name, which="real"):
    """the brute-force evaluation of the oracle's count matrix: the kept (text, class) pairs, the best class per text, the
    hits and the top texts per class -- whichever of them the entry point gives"""
    e = _scored(f, f._side(which)[1], score_model(f))
    top_n, top_text, top_score = e.top(TOP)
    kept = [e.kept_ptr.astype(np.int64), e.kept_class.view(np.int32), e.kept_score, e.best.view(np.int32)]
    top = [e.class_hits.astype(np.int64), top_n.view(np.int32), top_text.reshape(-1).view(np.int32), top_score.reshape(-1)]
    if name == "acm_gpu_score_matrix_device":
        return kept + [np.array([e.n_kept])]
    if name == "acm_gpu_score_top_device":
        return top
    return kept + top + [None]                           # (the four counts of the windowed scan: a scratch diagnostic among them)


def score_case(torch, f, name):
    L, h, N, T, CAP = binding.lib(), f.plan.h, f.N, f.T, sc.CAP
    sm = score_model(f)
    S = score_handle(f).h
    C = sm.n_classes
    FC = T * C
    want, other = _scored(f, f.rec, sm), _scored(f, f.rec_decoy, sm)
    assert 0 < want.n_kept <= FC and want.n_kept != other.n_kept
    kept_outs = {"kept_ptr": (T + 1, torch.int64), "kept_class": (FC, torch.int32), "kept_score": (FC, torch.int64), "best": (T, torch.int32)}
    top_outs = {"hits": (C, torch.int64), "top_n": (C, torch.int32), "top_text": (C * TOP, torch.int32), "top_score": (C * TOP, torch.int64)}

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
                       want=score_expected(f, name))
    if name == "acm_gpu_score_top_device":
        tb = L.acm_gpu_score_top_tmp_bytes(h, FC, C)
        gated = {"kept_ptr": (want.kept_ptr.astype(np.int64), other.kept_ptr.astype(np.int64)),
                 "kept_class": (_pad(want.kept_class, FC), _pad(other.kept_class, FC)), "kept_score": (_pad(want.kept_score, FC), _pad(other.kept_score, FC))}
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_score_top_device(h, p["kept_ptr"], p["kept_class"], p["kept_score"], FC, T, C, TOP, p["hits"], p["top_n"],
                                                                p["top_text"], p["top_score"], p["tmp"], tb, st),
                       gated, top_outs, tb, cut=top_cut, want=score_expected(f, name))
    tb = L.acm_gpu_score_tmp_bytes(h, S, sc.WINDOW, CAP, CAP, N, T, FC, TOP)
    off = f.d_off.data_ptr()
    return sc.Case(name, f.plan,
                   lambda p, st: L.acm_gpu_score_device(h, S, p["text"], N, off, T, sc.WINDOW, CAP, CAP, p["kept_ptr"], p["kept_class"], p["kept_score"], FC,
                                                        p["res"], p["best"], TOP, p["hits"], p["top_n"], p["top_text"], p["top_score"], p["res"] + 8,
                                                        p["res"] + 16, p["res"] + 24, p["tmp"], tb, st),
                   f._text(), dict(kept_outs, res=(4, torch.int64), **top_outs), tb,
                   cut=lambda x: kept_cut(x, x["res"][0]) + top_cut(x) + [x["res"]], want=score_expected(f, name))


# ---------------------------------------------------------------------------------------------- index
def index_longest(f):
    """a value of ACM_GPU_INDEX_LIST with lists of the real batch on either side of it"""
    lengths = np.unique(brute_force(_counts(f, f.rec), f.K).df)
    lengths = lengths[lengths > 0]
    assert lengths.size >= 2
    return int(lengths[(lengths.size - 1) // 2])


def _posted(e):
    return [e.post_ptr.astype(np.int64), e.post_text.view(np.int32), e.post_count.astype(np.int64)]


def index_expected(f, name, which="real", longest=None):
    """the brute-force transposition of the oracle's count matrix, and how many lists take the one-wave form and the wide
    one under ACM_GPU_INDEX_LIST = longest"""
    e = brute_force(_counts(f, f._side(which)[1]), f.K, BASE)
    if name == "acm_gpu_index_matrix_device":
        fast, wide = forms_of(e, index_longest(f) if longest is None else longest)
        return _posted(e) + [np.array([e.nnz, fast, wide])]
    if name == "acm_gpu_index_concat_device":
        return _posted(e) + [np.array([e.nnz])]
    return _posted(e) + [None]                           # (the counts of the windowed scan: a scratch diagnostic among them)


def index_case(torch, f, name, longest):
    """(call it, and run its case, with ACM_GPU_INDEX_LIST set to `longest`)"""
    L, h, N, T, K, CAP = binding.lib(), f.plan.h, f.N, f.T, f.K, sc.CAP
    counts, counts_decoy = _counts(f, f.rec), _counts(f, f.rec_decoy)
    want, other = brute_force(counts, K, BASE), brute_force(counts_decoy, K, BASE)
    fast, wide = forms_of(want, longest)
    assert fast > 0 and wide > 0 and T > longest and max(want.nnz, other.nnz) <= CAP
    outs = {"post_ptr": (K + 1, torch.int64), "post_text": (CAP, torch.int32), "post_count": (CAP, torch.int64)}

    def cut(x, n):
        return [x["post_ptr"], x["post_text"][:n], x["post_count"][:n]]
    if name == "acm_gpu_index_matrix_device":
        tb = L.acm_gpu_index_matrix_tmp_bytes(h, T, K, CAP)
        (rp, c, v), (rp2, c2, v2) = f._matrix(f.rec), f._matrix(f.rec_decoy)
        room = max(c.size, c2.size)
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_index_matrix_device(h, p["row_ptr"], p["col"], p["val"], T, K, BASE, p["post_ptr"], p["post_text"],
                                                                   p["post_count"], CAP, p["res"], p["res"] + 8, p["tmp"], tb, st),
                       {"row_ptr": (rp, rp2), "col": (_pad(c, room), _pad(c2, room)), "val": (_pad(v, room), _pad(v2, room))},
                       dict(outs, res=(3, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]],
                       want=index_expected(f, name, "real", longest))
    if name == "acm_gpu_index_concat_device":
        half = T // 2
        parts = [[brute_force(cut_rows(cn, 0, half), K, BASE), brute_force(cut_rows(cn, half, T), K, BASE + half)] for cn in (counts, counts_decoy)]
        assert all(p.nnz > 0 for pair in parts for p in pair)
        assert np.array_equal(concat_expected(*parts[0]).post_text, want.post_text)
        tb = L.acm_gpu_index_concat_tmp_bytes(h, K)
        gated = {}
        for i, side in enumerate(("a", "b")):
            real, decoy = parts[0][i], parts[1][i]
            gated[side + "_ptr"] = (real.post_ptr.astype(np.int64), decoy.post_ptr.astype(np.int64))
            gated[side + "_text"] = (_pad(real.post_text, CAP), _pad(decoy.post_text, CAP))
            gated[side + "_count"] = (_pad(real.post_count, CAP), _pad(decoy.post_count, CAP))
        return sc.Case(name, f.plan,
                       lambda p, st: L.acm_gpu_index_concat_device(h, p["a_ptr"], p["a_text"], p["a_count"], K, p["b_ptr"], p["b_text"], p["b_count"], K,
                                                                   p["post_ptr"], p["post_text"], p["post_count"], CAP, p["res"], p["tmp"], tb, st),
                       gated, dict(outs, res=(1, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]],
                       want=index_expected(f, name, "real", longest))
    tb = L.acm_gpu_index_tmp_bytes(h, sc.WINDOW, CAP, CAP, N, T, K, CAP)
    off = f.d_off.data_ptr()
    return sc.Case(name, f.plan,
                   lambda p, st: L.acm_gpu_index_device(h, p["text"], N, off, T, sc.WINDOW, CAP, CAP, K, BASE, p["post_ptr"], p["post_text"], p["post_count"],
                                                        CAP, p["res"], p["res"] + 32, p["res"] + 8, p["res"] + 16, p["res"] + 24, p["tmp"], tb, st),
                   f._text(), dict(outs, res=(6, torch.int64)), tb, cut=lambda x: cut(x, x["res"][0]) + [x["res"]], want=index_expected(f, name, "real", longest))


# ---------------------------------------------------------------------------------------------- near
def near_groups(f):
    """the two keywords the batch holds most often (the chain set's) near each other, in either order"""
    a, b = (int(x) for x in f.chainset.terms[:2, 0])
    return [([a, b], 40, 0), ([b, a], 25, 1)]


def near_handle(f):
    """the groups compiled on f.plan as it is now, once"""
    if "near" not in f.handles:
        f.handles["near"] = f.plan.near(near_groups(f))
    return f.handles["near"]


def near_expected(f, name, which="real"):
    """NEAR of the batch's first n records, or (the fused form) of the records of the buffer as one text, and the counts"""
    return [np.asarray(w) for w in f._want_join(which, name == "acm_gpu_scan_near_device", lambda rec, text: near(rec, near_groups(f), f.N, f.off))]


def near_case(torch, f, name):
    most = int(near_handle(f).info()["max_postings"])
    case = f._join_records(name, "near", most) if name == "acm_gpu_near_records_device" else f._join_scan(name, "near", most)
    case.want = near_expected(f, name)
    assert case.want[0].shape[0] >= 16
    return case


def expected(f, name, which="real", longest=None):
    """the expected value of any of ENTRIES, without a device"""
    if name in SEGMENT:
        return segment_expected(f, name, which)
    if name in SCORE:
        return score_expected(f, name, which)
    if name in INDEX:
        return index_expected(f, name, which, longest)
    assert name in NEAR, name
    return near_expected(f, name, which)


def case(torch, f, name, longest=None):
    """the case of any of ENTRIES"""
    if name in SEGMENT:
        return segment_case(torch, f, name)
    if name in SCORE:
        return score_case(torch, f, name)
    if name in INDEX:
        return index_case(torch, f, name, index_longest(f) if longest is None else longest)
    assert name in NEAR, name
    return near_case(torch, f, name)
