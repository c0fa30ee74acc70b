"""Keywords within edit distance k on the GPU (acm_gpu_edit_*, acm_gpu_scan_edit_*, acm_scan_edit; csrc/dev_edit.h).
The expected answer is always the definition of EDIT in Python over the ORACLE's records (tests/edit_cases.py: a
free-start Sellers pass with the largest-start rule, then the seed condition) -- never the library's own scan or
verification.  The second derivation from the text alone (edit_scan: a plain Levenshtein distance for every end
and start) is affordable for a few hundred symbols: the many-seeds cases, the cases at the buffer's ends and the
head of the striding case use it; the main case is compared with the definition without its seed condition
instead, the cuts being canonical.  All comparisons are exact, order, lengths and distances included.  Texts are
a few KiB; one case has more records than the capped grid has groups of tiles of 64, so that blocks stride over
tiles."""
import functools

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.approx_cases import compile_targets, same
from tests.edit_cases import edit_scan, edits, plant, seeds_of
from tests.tally_cases import PATH_GPU, kind

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INELIGIBLE, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, binding.ACM_GPU_E_INELIGIBLE, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
SENTINEL = 0x0123456789ABCDEF
LENGTHS = (15, 16, 17, 31, 32, 33, 64, 65, 300)
AY = np.frombuffer(b"abcdefghijklmnopqrstuvwxy", np.uint8)
Z = ord("z")                                                       # in no target


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _dev(torch, arr):
    a = np.frombuffer(bytes(arr), dtype=np.uint8) if isinstance(arr, (bytes, bytearray)) else np.ascontiguousarray(arr)
    a = a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])
    return torch.from_numpy(a.copy()).cuda()


def _rec_dev(torch, rec, room=None, fill=None):
    a = np.zeros(max(rec.size if room is None else room, 1), po.RECORD_DTYPE)
    if fill is not None:
        a["end_pos"] = fill
    a[:rec.size] = rec
    return torch.from_numpy(a.view(np.int64).reshape(-1, 2).copy()).cuda()


def _rec_host(t, n):
    return np.frombuffer(t[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()


def _dist_host(t, n):
    return t[:n].cpu().numpy().astype(np.uint32)


def _sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(DTYPE[sb])


def _records(kws, text, sb=1):
    """the oracle's records of a text in symbols of sb bytes (canonical order)"""
    o = po.Oracle(sb, po.MEYER85)
    for kw in kws:
        o.add_keyword(np.array(kw, DTYPE[sb]))
    text = np.ascontiguousarray(text, DTYPE[sb])
    return o.scan(text) if text.size else np.zeros(0, po.RECORD_DTYPE)


def _join(plan, rec, approx_set, dev_text, **kw):
    """Plan.edit_records on the records `rec` (host): ((the matches, their distances) (host), the count)"""
    torch = __import__("torch")
    out, dist, cnt = plan.edit_records(_rec_dev(torch, rec), rec.size, approx_set, dev_text, **kw)
    n = int(cnt.item())
    return (_rec_host(out, min(n, out.shape[0])), _dist_host(dist, min(n, out.shape[0]))), n


def _scan(plan, dev, approx_set, capacity, **kw):
    """Plan.scan_edit: ((the matches, their distances) (host), the count, the scan's count)"""
    out, dist, cnt, found, _ = plan.scan_edit(dev, approx_set, capacity=capacity, **kw)
    n = int(cnt.item())
    return (_rec_host(out, min(n, out.shape[0])), _dist_host(dist, min(n, out.shape[0]))), n, int(found.item())


def _moved(want, by):
    rec = want[0].copy()
    rec["end_pos"] += by
    return rec, want[1]


def _budget(L, max_k):
    return min(max_k, L // 4)


@functools.lru_cache(maxsize=None)
def _letters(max_k):
    """(targets, budgets, text, planted) as bytes: targets of the LENGTHS over a-y with k = min (max_k, L / 4).  The
    text: two symbols of noise and an exact copy of target 0 (within k symbols of the buffer's start: the band is
    clipped at lo); per target, copies with 0 to k + 1 edits of all three kinds (edit_cases.plant) between noise;
    copies of target 3 with its first and its last symbol substituted, deleted and doubled; an exact copy of
    target 2 and one symbol of noise (within k symbols of the buffer's end).  planted: (target, edits, begin, end)."""
    rng = np.random.default_rng(1975 + max_k)
    targets = [bytes(rng.choice(AY, size=n)) for n in LENGTHS]
    ks = [_budget(n, max_k) for n in LENGTHS]
    parts, planted, at = [], [], 0

    def put(piece, w=None, d=None):
        nonlocal at
        parts.append(bytes(piece))
        if w is not None:
            planted.append((w, d, at, at + len(piece)))
        at += len(piece)
    put(rng.choice(AY, size=2))
    put(targets[0], 0, 0)
    for w, t in enumerate(targets):
        for d in range(ks[w] + 2):
            put(rng.choice(AY, size=int(rng.integers(3, 20))))
            put(plant(rng, t, d, Z), w, d)
    t = targets[3]
    for copy in (bytes([Z]) + t[1:], t[1:], t[:1] + t, t[:-1] + bytes([Z]), t[:-1], t + t[-1:]):
        put(rng.choice(AY, size=12))
        put(copy, 3, 1)
    put(rng.choice(AY, size=40))
    put(targets[2], 2, 0)
    put(rng.choice(AY, size=1))
    return targets, ks, b"".join(parts), planted


@functools.lru_cache(maxsize=None)
def _main(max_k, sb):
    """(targets, budgets, text, the plain-Python cut, the oracle's records, EDIT of them) in symbols of sb bytes; in wider
    symbols one letter of the exact copy of target 1 loses its high byte: an edit no low-byte compare sees.  The cuts
    are canonical and the record set is full, so the definition says the same without its seed condition."""
    t8, ks, text8, planted = _letters(max_k)
    targets = [_sym(t, sb) for t in t8]
    text = _sym(text8, sb)
    if sb > 1:
        at = [p for p in planted if p[0] == 1 and p[1] == 0][0][2]
        text[at + 5] ^= DTYPE[sb](HIGH[sb])
    kws, terms = compile_targets(targets, ks)
    rec = _records(kws, text, sb)
    want = edits(rec, text, targets, ks, terms)
    same(want, edits(None, text, targets, ks, terms, seeded=False), "the definition, with and without its seed condition")
    return targets, ks, text, (kws, terms), rec, want


def _machine(sb, targets, ks, cut):
    m = acm.Machine(sb)
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    kws, terms = cut
    assert [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws and aset.terms.tolist() == [list(t) for p in terms for t in p]
    return m, aset


@pytest.mark.parametrize("max_k", [3, 7, 15])
def test_the_case_is_not_trivial(max_k):
    targets, ks, text, (kws, terms), rec, want = _main(max_k, 1)
    planted = _letters(max_k)[3]
    w, d, end, length = want[0]["keyword_id"], want[1], want[0]["end_pos"], want[0]["length"]
    L_of = np.array(LENGTHS)[w]
    print("max_k %d: symbols %d, keywords %d, records %d, matches %d, distances %s, shorter / equal / longer %d / %d / %d" % (
        max_k, text.size, len(kws), rec.size, w.size, np.bincount(d).tolist(), np.count_nonzero(length < L_of), np.count_nonzero(length == L_of),
        np.count_nonzero(length > L_of)))
    assert text.size < 16384 and max(ks) == max_k and np.all(d <= np.array(ks)[w])
    assert np.any(length < L_of) and np.any(length > L_of) and set(range(max_k + 1)) <= set(d.tolist())
    for t, n_edits, begin, stop in planted:
        here = (w == t) & (end >= begin + LENGTHS[t] // 2) & (end < stop + ks[t])
        if n_edits <= ks[t]:                                                      # the copy ends as the target does: its own end is reported
            assert np.any(d[here & (end == stop - 1)] <= n_edits) or (t == 3 and n_edits == 1 and np.any(d[here] == 1)), (t, n_edits)
        else:                                                                     # the copy with k + 1 edits must not appear
            assert not np.any(here), (t, n_edits, want[0][here])
    # the ownership rule's hard case: the exact copy of the longest target is seeded by every piece at every end within its budget
    t, n_edits, begin, stop = [p for p in planted if p[0] == 8 and p[1] == 0][0]
    around = (w == 8) & (end >= stop - 1 - ks[8]) & (end <= stop - 1 + ks[8])
    assert np.count_nonzero(around) == 2 * ks[8] + 1
    assert seeds_of(rec, (0, text.size), stop - 1, 300, ks[8], terms[8]) == ks[8] + 1
    assert min(seeds_of(rec, (0, text.size), int(e), 300, ks[8], terms[8]) for e in end[around]) >= 1


@pytest.mark.parametrize("max_k", [3, 7, 15])
@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_every_group_width_on_every_symbol_size(torch_cuda, sb, max_k):
    targets, ks, text, cut, rec, want = _main(max_k, sb)
    m, aset = _machine(sb, targets, ks, cut)
    aset.check_edit()
    plan = m.plan(0)
    dev = _dev(torch_cuda, text)
    A = plan.approx_create(aset)
    info = A.info()
    assert info["targets"] == len(targets) and info["longest"] == 300 and info["max_k"] == max_k
    got, n, found = _scan(plan, dev, A, rec.size)
    assert found == rec.size and n == want[0].size
    same(got, want, (sb, max_k))
    # the verification alone on the oracle's records, with the compiled set and with a set compiled for the call
    same(_join(plan, rec, A, dev)[0], want, (sb, max_k))
    same(_join(plan, rec, aset, dev)[0], want, (sb, max_k))
    # nonzero pos_base
    shifted = rec.copy()
    shifted["end_pos"] += 5000
    same(_scan(plan, dev, A, rec.size, pos_base=5000)[0], _moved(want, 5000), sb)
    same(_join(plan, shifted, A, dev, pos_base=5000)[0], _moved(want, 5000), sb)
    # the text at an address that is no multiple of 16 (for bytes: an odd one)
    room = torch_cuda.zeros(text.size + 1, dtype=dev.dtype, device="cuda")
    room[1:] = dev
    assert room[1:].data_ptr() % 16 == sb and room[1:].is_contiguous()
    same(_join(plan, rec, A, room[1:])[0], want, sb)
    same(_scan(plan, room[1:], A, rec.size)[0], want, sb)
    # host memory in, blocking; the machine's own call on the GPU path
    same(plan.scan_edit_host(text, aset), want, sb)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_edit_host(text, aset, out_capacity=want[0].size - 1)
    assert e.value.code == E_OVERFLOW
    same(m.scan_edit(text, aset), want, sb)
    assert m.scan_path == PATH_GPU
    with pytest.raises(acm.ACMError) as e:
        m.scan_edit(text, aset, out_capacity=want[0].size - 1)
    assert e.value.code == E_OVERFLOW
    # an empty text, a text without a record
    assert plan.scan_edit_host(np.zeros(0, DTYPE[sb]), aset)[0].size == 0
    got, n, found = _scan(plan, _dev(torch_cuda, _sym(b"q" * 3000, sb)), A, 16)
    assert (n, found) == (0, 0)
    A.close()
    plan.status()


def test_sets_the_edit_calls_do_not_take(torch_cuda):
    torch, L = torch_cuda, acm.lib()
    m = acm.Machine(1)
    wide = binding.ApproxSet.from_targets(m, [b"abcdefghijklmnopqrstuvwxyzabcdefghijklmnopqrstuvwxyz"], 16)   # k = 16
    full = binding.ApproxSet([b"abcd"], [4], [[(0, 0, 3)]])                      # k = L (keyword 0 is `abc`)
    fine = binding.ApproxSet.from_targets(m, [b"abcdefgh"], 1)
    plan = m.plan(0)
    one = torch.zeros(64, dtype=torch.int64, device="cuda")
    for aset in (wide, full):
        aset.check(m.nb_keywords)                                                 # APPROX takes it
        with pytest.raises(acm.ACMError):
            aset.check_edit(m.nb_keywords)
        A = plan.approx_create(aset)                                              # (the set cannot know which call it is for)
        assert L.acm_gpu_approx_tmp_bytes(plan.h, A.h, 64, 64, 0) > 0
        assert L.acm_gpu_edit_tmp_bytes(plan.h, A.h, 64, 64, 0) == 0 and L.acm_gpu_scan_edit_tmp_bytes(plan.h, A.h, 64, 64, 64, 0) == 0
        assert L.acm_gpu_edit_records_device(plan.h, A.h, one.data_ptr(), 2, None, one.data_ptr(), 8, 0, None, 0, one.data_ptr() + 256, None, 1,
                                             one.data_ptr() + 128, one.data_ptr(), 512, None) == E_ARG
        assert L.acm_gpu_scan_edit_device(plan.h, A.h, one.data_ptr(), 8, 0, None, 0, 4, one.data_ptr(), None, 1, one.data_ptr(), one.data_ptr() + 8,
                                          one.data_ptr(), 512, None) == E_ARG
        for call in (plan.scan_edit_host, m.scan_edit):
            with pytest.raises(acm.ACMError) as e:
                call(b"abcdefgh", aset)
            assert e.value.code == E_ARG
        A.close()
    A = plan.approx_create(fine)
    assert L.acm_gpu_edit_tmp_bytes(plan.h, A.h, 64, 64, 0) > 0 and L.acm_gpu_scan_edit_tmp_bytes(plan.h, A.h, 64, 64, 64, 0) > 0
    assert L.acm_gpu_edit_tmp_bytes(plan.h, A.h, 1 << 31, 0, 0) == 0 and L.acm_gpu_edit_tmp_bytes(plan.h, A.h, 64, 1 << 31, 0) == 0
    assert L.acm_gpu_edit_tmp_bytes(plan.h, None, 64, 64, 0) == 0
    A.close()
    plan.status()


def _small(torch, target, k, text, offsets=None, scan_too=True):
    """one byte target with the canonical cut over a small byte text: the definition, edit_scan and every GPU call agree"""
    kws, terms = compile_targets([target], [k])
    rec = _records(kws, np.frombuffer(text, np.uint8))
    want = edits(rec, text, [target], [k], terms, offsets)
    same(want, edit_scan(text, [target], [k], offsets), ("the two derivations", target, k, text))
    m = acm.Machine(1)
    aset = binding.ApproxSet.from_targets(m, [target], k)
    plan = m.plan(0)
    dev = _dev(torch, text)
    d_off = _dev(torch, np.asarray(offsets, np.int64)) if offsets is not None else None
    same(_join(plan, rec, aset, dev, offsets=d_off)[0], want, (target, k, text))
    if scan_too:
        same(plan.scan_edit_host(np.frombuffer(text, np.uint8), aset, offsets=offsets), want, (target, k, text))
    plan.status()
    return want, rec, terms


def test_many_seeds_per_match(torch_cuda):
    """the ownership rule's small hard cases (the second derivation is affordable here)"""
    want, rec, terms = _small(torch_cuda, b"abab", 1, b"abababab")                # periodic; two identical pieces share one keyword
    assert terms == [[(0, 0, 2), (0, 2, 2)]]
    assert want[0]["end_pos"].tolist() == [2, 3, 4, 5, 6, 7] and want[1].tolist() == [1, 0, 1, 0, 1, 0]
    assert max(seeds_of(rec, (0, 8), int(e), 4, 1, terms[0]) for e in want[0]["end_pos"]) >= 3
    _small(torch_cuda, b"abab", 1, b"xxababxx")
    _small(torch_cuda, b"abab", 3, b"babababbbabaabab" * 4)
    _small(torch_cuda, b"aaaaaaaa", 3, b"aaaaaaaaaaaaaaaaaaaabaaaaaaaaaaaa")             # four identical pieces, every end seeded many times
    want, rec, terms = _small(torch_cuda, b"abcabcabcabcabcabc", 5, b"abcabcabcabcabcabcabcabcabc" * 3)   # G = 32
    assert max(seeds_of(rec, (0, 81), int(e), 18, 5, terms[0]) for e in want[0]["end_pos"]) >= 12


def test_copies_at_the_buffers_two_ends(torch_cuda):
    rng = np.random.default_rng(5)
    t = bytes(rng.choice(AY, size=24))
    noise = bytes(rng.choice(AY, size=30))
    for k in (1, 3, 6):
        for lead in (0, 1, k):                                                    # a copy within k symbols of each end: the band is clipped
            _small(torch_cuda, t, k, noise[:lead] + t + noise + t + noise[:lead], scan_too=False)
        _small(torch_cuda, t, k, t[2:] + noise + t[:-2], scan_too=False)          # an edit that the buffer's end makes
        _small(torch_cuda, t, k, t[-10:] + noise + t[:10])                        # seeds that point in front of the buffer and behind it
    _small(torch_cuda, t, 6, t)
    _small(torch_cuda, t, 6, t[:20])
    _small(torch_cuda, t, 6, t[3:9])


def test_text_boundaries_of_a_packed_batch(torch_cuda):
    targets, ks, text, cut, rec, want = _main(3, 1)
    kws, terms = cut
    planted = _letters(3)[3]
    exact = {w: (b, e) for w, d, b, e in planted if d == 0}
    inside = exact[4][0] + 11                                                     # a cut inside the exact copy of target 4
    at_end = exact[5][1]                                                          # a text that ends exactly with the copy of target 5
    off = np.array(sorted([0, 0, 9, inside, at_end, at_end, 3000, text.size, text.size]), np.uint64)
    cut_want = edits(rec, text, targets, ks, terms, off)
    same(cut_want, edits(None, text, targets, ks, terms, off, seeded=False), "the definition, with and without its seed condition")
    whole = {tuple(int(x) for x in r) for r in want[0]}
    kept = {tuple(int(x) for x in r) for r in cut_want[0]}
    assert (exact[4][1] - 1, 32, 4) in whole - kept and (at_end - 1, 33, 5) in kept and 0 < len(kept) < len(whole)
    assert not any(r[2] == 4 and exact[4][0] <= r[0] < exact[4][1] + 3 for r in kept)     # neither half is within the budget: nothing reaches across
    assert any(inside - r[2] < r[0] - r[1] + 1 < inside <= r[0] for r in map(tuple, rec))  # the ordered scan hands over records that span the cut
    m, aset = _machine(1, targets, ks, cut)
    plan = m.plan(0)
    dev, d_off = _dev(torch_cuda, text), _dev(torch_cuda, off.astype(np.int64))
    same(_join(plan, rec, aset, dev, offsets=d_off)[0], cut_want)
    same(_join(plan, rec, aset, dev)[0], want)
    got, n, found = _scan(plan, dev, aset, rec.size, offsets=d_off)
    assert found == rec.size
    same(got, cut_want)
    same(plan.scan_edit_host(text, aset, offsets=off), cut_want)
    same(m.scan_edit(text, aset, offsets=off), cut_want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_edit_host(text, aset, offsets=[0, 9, 5, text.size])
    assert e.value.code == E_ARG
    plan.status()                                                                 # a seed that points outside its text is no error
    # a match that is within the budget only by reaching across a cut is absent: `abcdefgh` | `ijkl`, k = 2
    want, _, _ = _small(torch_cuda, b"abcdefghijkl", 2, b"xxabcdefghijklxx", offsets=np.array([0, 10, 16], np.uint64))
    assert want[0].size == 0
    want, _, _ = _small(torch_cuda, b"abcdefghijkl", 2, b"xxabcdefghijklxx", offsets=np.array([0, 12, 12, 16], np.uint64))
    assert want[0]["end_pos"].tolist() == [11] and want[1].tolist() == [2]      # `abcdefghij` alone is within 2; nothing in the second text


@pytest.mark.parametrize("name", ["dense", "gram", "starts"])
def test_scan_edit_on_plan_kinds(torch_cuda, monkeypatch, kat, name):
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    sb = m.sym_size
    rng = np.random.default_rng(75)
    body = text[:4096].astype(DTYPE[sb])
    targets = [body[100:120].copy(), body[1000:1033].copy(), body[2000:2007].copy()]
    ks = [2, 3, 1]
    stranger = int(250 if sb == 1 else 0xFFFFF0)                                  # (in no target)
    planted = []
    for t, k in zip(targets, ks):
        for d in range(k + 2):
            planted += [np.array(plant(rng, [int(x) for x in t], d, stranger), DTYPE[sb]), body[3000:3011]]
    buf = np.concatenate(planted + [body])
    before = m.nb_keywords
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    for i in range(before, m.nb_keywords):                                        # the oracle gets the new pieces under the same ids
        o.add_keyword(np.array(m.keyword(i)[0], DTYPE[sb]))
    assert o.nb_keywords == m.nb_keywords
    terms = [[tuple(int(x) for x in aset.terms[i]) for i in range(int(aset.tgt_ptr[w]), int(aset.tgt_ptr[w + 1]))] for w in range(len(targets))]
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    rec = o.scan(buf)
    want = edits(rec, buf, targets, ks, terms)
    same(want, edits(None, buf, targets, ks, terms, seeded=False), "the definition, with and without its seed condition")
    print("%s: records %d, matches %d, distances %s" % (name, rec.size, want[0].size, np.bincount(want[1]).tolist()))
    assert want[0].size >= 2 + 3 + 4 + 3 and np.count_nonzero(want[1]) >= 6
    got, n, found = _scan(plan, _dev(torch_cuda, buf), aset, rec.size)
    assert found == rec.size
    same(got, want, name)
    plan.status()


def test_plans_that_intern_8_byte_symbols_are_taken_and_class_plans_refused(torch_cuda, monkeypatch, kat):
    m, o, text, make_plan, plan_ok, _ = kind("u64", monkeypatch, kat)
    body = text[:3000]
    targets, ks = [body[500:517].copy()], [2]
    buf = body.copy()
    buf[1000:1017] = targets[0]
    buf[1003] ^= np.uint64(1 << 60)                                               # outside the dictionary's symbols: interned to `unknown`
    buf[1500:1516] = np.delete(targets[0], 7)                                     # a deletion ...
    buf[1501] = np.uint64(12345)                                                  # ... and a substitution
    before = m.nb_keywords
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    for i in range(before, m.nb_keywords):
        o.add_keyword(np.array(m.keyword(i)[0], np.uint64))
    terms = [[tuple(int(x) for x in t) for t in aset.terms]]
    plan = make_plan(0)
    rec = o.scan(buf)
    want = edits(rec, buf, targets, ks, terms)
    same(want, edits(None, buf, targets, ks, terms, seeded=False), "the definition, with and without its seed condition")
    assert {0, 1, 2} <= set(want[1].tolist()) and (1515, 16, 0) in [tuple(int(x) for x in r) for r in want[0]]
    got, n, found = _scan(plan, _dev(torch_cuda, buf), aset, rec.size)
    assert found == rec.size
    same(got, want)
    plan.status()
    mc, _, _, make_classes, _, _ = kind("classes", monkeypatch, kat)
    classes = make_classes(0)
    with pytest.raises(acm.ACMError) as e:
        classes.scan_edit_host(np.frombuffer(b"mrs dalloway", np.uint8), binding.ApproxSet([b"dalloway"], [1], [[(5, 0, 8)]]))
    assert e.value.code == E_INELIGIBLE                                           # verification is bitwise on the caller's text
    A, L = plan.approx_create(aset), acm.lib()
    assert L.acm_gpu_edit_tmp_bytes(plan.h, A.h, 64, 64, 0) > 0 and L.acm_gpu_scan_edit_tmp_bytes(plan.h, A.h, 64, 64, 64, 0) > 0
    assert L.acm_gpu_edit_tmp_bytes(classes.h, A.h, 64, 64, 0) == 0 and L.acm_gpu_scan_edit_tmp_bytes(classes.h, A.h, 64, 64, 64, 0) == 0
    one = torch_cuda.zeros(64, dtype=torch_cuda.int64, device="cuda")
    assert L.acm_gpu_scan_edit_device(classes.h, A.h, one.data_ptr(), 8, 0, None, 0, 4, one.data_ptr(), None, 1, one.data_ptr(), one.data_ptr() + 8,
                                      one.data_ptr(), 512, None) == E_ARG
    A.close()


def test_more_records_than_the_grid_has_groups(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles"""
    monkeypatch.setenv("ACM_GPU_EDIT_TILE", "64")
    targets, ks = [b"abbab", b"babab", b"aab"], [1, 1, 0]
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = ((8 * cus + 3) * 64 + 65) * 3 // 2                                        # (three records per four symbols)
    text = bytes(np.random.default_rng(8).choice(np.frombuffer(b"ab", np.uint8), size=n))
    m = acm.Machine(1)
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    kws, terms = compile_targets(targets, ks)
    rec = _records(kws, np.frombuffer(text, np.uint8))
    assert rec.size > (8 * cus + 2) * 64 + 65
    want = edits(None, text, targets, ks, terms, seeded=False)                    # (canonical cuts, the full record set)
    head = rec[rec["end_pos"] < 400]
    part = edits(head, text[:400], targets, ks, terms)
    same(part, edit_scan(text[:400], targets, ks), "the two derivations, where the loop is affordable")
    same(part, edits(None, text[:400], targets, ks, terms, seeded=False), "with and without the seed condition")
    plan = m.plan(0)
    got, cnt = _join(plan, rec, aset, _dev(torch_cuda, text), out_capacity=want[0].size)
    same(got, want)
    assert n // 4 < want[0].size
    plan.status()


def test_out_capacity_counts_on_the_device_and_overflow(torch_cuda):
    torch = torch_cuda
    targets, ks, text, cut, rec, want = _main(3, 1)
    m, aset = _machine(1, targets, ks, cut)
    plan = m.plan(0)
    A = plan.approx_create(aset)
    dev = _dev(torch, text)
    total = want[0].size
    assert total > 30
    sentinel = np.zeros(total + 8, po.RECORD_DTYPE)
    sentinel["end_pos"], sentinel["length"], sentinel["keyword_id"] = SENTINEL, 7, 7

    def join(out_capacity, count=None, room=None):
        d_out = _rec_dev(torch, sentinel)
        d_dist = torch.full((total + 8,), 0x5A5A, dtype=torch.int32, device="cuda")
        d_rec = _rec_dev(torch, rec, room, fill=SENTINEL)
        out, dist, cnt = plan.edit_records(d_rec, rec.size if room is None else room, A, dev, out=d_out, dist=d_dist, out_capacity=out_capacity, count=count)
        return _rec_host(d_out, sentinel.size), _dist_host(d_dist, total + 8), int(cnt.item())
    # the exact room; one short: the count is exact and nothing is written at or behind out_capacity; no room: the count alone
    out, dist, n = join(total)
    assert n == total and np.array_equal(out[total:], sentinel[total:]) and np.all(dist[total:] == 0x5A5A)
    same((out[:n], dist[:n]), want)
    out, dist, n = join(total - 1)
    assert n == total and np.array_equal(out, sentinel) and np.all(dist == 0x5A5A)
    out, dist, n = join(0)
    assert n == total and np.array_equal(out, sentinel) and np.all(dist == 0x5A5A)
    out, dist, n = join(1)
    assert n == total and np.array_equal(out, sentinel) and np.all(dist == 0x5A5A)
    out, dist, n = join(total + 5)                                                # more room than matches: the padding of the order is not seen
    assert n == total and np.array_equal(out[total:], sentinel[total:]) and np.all(dist[total:] == 0x5A5A)
    same((out[:n], dist[:n]), want)
    # the default room cannot overflow: n x max_postings x (2 max_k + 1)
    info = A.info()
    out, dist, cnt = plan.edit_records(_rec_dev(torch, rec), rec.size, A, dev)
    assert out.shape[0] == rec.size * info["max_postings"] * (2 * info["max_k"] + 1) and int(cnt.item()) == total
    # d_n given: n is the room of the records
    room = rec.size + 100
    out, dist, n = join(total, count=torch.tensor([rec.size], dtype=torch.int64, device="cuda"), room=room)
    same((out[:n], dist[:n]), want)
    # a scan that overflowed: *d_n > room -- *d_count = 0 and nothing is written
    out, dist, n = join(total, count=torch.tensor([room + 1], dtype=torch.int64, device="cuda"), room=room)
    assert n == 0 and np.array_equal(out, sentinel) and np.all(dist == 0x5A5A)
    # the fused call with too little room for the scan's records: no match, *d_found suffices on repeat
    got, n, found = _scan(plan, dev, A, rec.size - 1, out_capacity=total)
    assert n == 0 and found == rec.size
    got, n, found = _scan(plan, dev, A, found, out_capacity=total)
    assert found == rec.size
    same(got, want)
    got, n, found = _scan(plan, dev, A, 0, out_capacity=total)                    # no room at all: the scan's count
    assert n == 0 and found == rec.size
    got, n, found = _scan(plan, dev, A, rec.size, out_capacity=total - 1)         # the records fit, the matches do not
    assert n == total and found == rec.size
    # dist may be NULL; refused calls
    L = acm.lib()
    d_rec, d_out, cnt = _rec_dev(torch, rec), _rec_dev(torch, sentinel), torch.zeros(1, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_edit_tmp_bytes(plan.h, A.h, rec.size, total, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call(approx_h=A.h, records=d_rec.data_ptr(), n=rec.size, text_ptr=dev.data_ptr(), out=d_out.data_ptr(), cap=total, count=cnt.data_ptr(),
             scratch=tmp.data_ptr(), tmp_bytes=tb):
        return L.acm_gpu_edit_records_device(plan.h, approx_h, records, n, None, text_ptr, text.size, 0, None, 0, out, None, cap, count, scratch, tmp_bytes, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == total and np.array_equal(_rec_host(d_out, total), want[0])
    assert call(approx_h=None) == E_ARG and call(records=None) == E_ARG and call(text_ptr=None) == E_ARG and call(out=None) == E_ARG
    assert call(count=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(cap=1 << 31) == E_ARG and call(out=d_rec.data_ptr()) == E_ARG     # d_out overlapping d_records
    A.close()
    plan.status()


def test_offsets_that_break_the_contract_match_nothing(torch_cuda):
    torch = torch_cuda
    targets, ks, text, cut, rec, want = _main(3, 1)
    m, aset = _machine(1, targets, ks, cut)
    n = text.size
    sentinel = np.zeros(want[0].size, po.RECORD_DTYPE)
    sentinel["end_pos"] = SENTINEL
    dev = _dev(torch, text)
    for what, off in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]), ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n])):
        plan = m.plan(0)
        plan.status()
        d_out = _rec_dev(torch, sentinel)
        out, dist, cnt = plan.edit_records(_rec_dev(torch, rec), rec.size, aset, dev, offsets=_dev(torch, np.array(off, np.int64)), out=d_out)
        assert int(cnt.item()) == 0, what
        assert np.array_equal(_rec_host(d_out, sentinel.size), sentinel), what
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_records_that_break_the_contract_are_skipped_and_reported(torch_cuda):
    targets, ks, text, cut, rec, want = _main(3, 1)
    m, aset = _machine(1, targets, ks, cut)
    pos_base = 1000
    shifted = rec.copy()
    shifted["end_pos"] += pos_base
    dev = _dev(torch_cuda, text)
    kid = 0                                                                       # (a keyword that seeds targets: the record would be looked at)
    bad = {"a start below pos_base": (pos_base + 1, 4, kid), "a length of 0": (pos_base + 20, 0, kid), "beyond the buffer": (pos_base + text.size, 1, kid),
           "below pos_base": (pos_base - 1, 1, kid), "far beyond": (1 << 62, 3, kid)}
    for what, triple in bad.items():
        plan = m.plan(0)
        plan.status()
        mixed = np.concatenate([shifted, np.array([triple], po.RECORD_DTYPE)])
        mixed = mixed[np.lexsort((-mixed["length"].astype(np.int64), mixed["end_pos"]))]   # canonical order with the stranger in it
        same(_join(plan, mixed, aset, dev, pos_base=pos_base)[0], _moved(want, pos_base), what)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_typos_of_six_words_of_the_novel(torch_cuda, novel_bytes):
    text = bytearray(novel_bytes[:8192])
    at = bytes(text).index(b"Dalloway")
    del text[at + 3]                                                              # `Daloway`: APPROX never reports it at k = 1
    text = bytes(text)
    words = [b"Clarissa", b"Dalloway", b"would", b"there", b"then", b"morning"]
    for k in (1, 2):
        ks = [k] * len(words)
        m = acm.Machine(1)
        aset = binding.ApproxSet.from_targets(m, words, k)
        kws, terms = compile_targets(words, ks)
        rec = _records(kws, np.frombuffer(text, np.uint8))
        want = edits(rec, text, words, ks, terms)
        same(want, edits(None, text, words, ks, terms, seeded=False), "the definition, with and without its seed condition")
        per = np.bincount(want[0]["keyword_id"], minlength=len(words))
        print("k = %d: matches per word %s, distances %s" % (k, per.tolist(), np.bincount(want[1]).tolist()))
        assert np.all(per >= 2) and (at + 6, 7, 1) in [tuple(int(x) for x in r) for r in want[0]]
        assert (at + 6, 7, 1) not in [tuple(int(x) for x in r) for r in m.scan_approx(text, aset)[0]]
        plan = m.plan(0)
        got, n, found = _scan(plan, _dev(torch_cuda, text), aset, rec.size)
        assert found == rec.size
        same(got, want, k)
        same(m.scan_edit(text, aset), want, k)
        plan.status()
