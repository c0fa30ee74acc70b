"""Keywords with up to k mismatches on the GPU (acm_gpu_approx_*, acm_gpu_scan_approx_*, acm_scan_approx;
csrc/dev_approx.h).  The expected answer is always the definition of APPROX in plain Python over the ORACLE's or
tests/brute.py's records (tests/approx_cases.py) and, the cuts being canonical, a second derivation from the text
alone (a brute-force Hamming scan with numpy) -- never the library's own scan or join.  All comparisons are exact,
order and distances included.  Texts are a few KiB; one case has more records than the capped grid has groups of
tiles of 64, so that blocks stride over tiles."""
import ctypes as C
import functools

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests.approx_cases import approx, brute, compile_targets, hamming_scan, oracle_records, same, seeds_of
from tests.batch_cases import broken_last_pair
from tests.tally_cases import PATH_GPU, kind

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INELIGIBLE, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, binding.ACM_GPU_E_INELIGIBLE, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
SENTINEL = 0x0123456789ABCDEF
LENGTHS = (15, 16, 17, 31, 32, 33, 300)                            # around the rounds of a 16-lane group
TIES = [b"abcdefgh", b"abcdefgx", b"zabcdefgh"]                    # equal and different lengths that end at one symbol


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


def _join(plan, rec, approx_set, dev_text, **kw):
    """Plan.approx_records on the records `rec` (host): ((the matches, their distances) (host), the count)"""
    torch = __import__("torch")
    out, dist, cnt = plan.approx_records(_rec_dev(torch, rec), rec.size, approx_set, dev_text, **kw)
    n = int(cnt.item())
    return (_rec_host(out, min(n, out.shape[0])), _dist_host(dist, min(n, out.shape[0]))), n


def _scan(plan, dev, approx_set, capacity, **kw):
    """Plan.scan_approx: ((the matches, their distances) (host), the count, the scan's count)"""
    out, dist, cnt, found, _ = plan.scan_approx(dev, approx_set, capacity=capacity, **kw)
    n = int(cnt.item())
    return (_rec_host(out, min(n, out.shape[0])), _dist_host(dist, min(n, out.shape[0]))), n, int(found.item())


def _moved(want, by):
    rec = want[0].copy()
    rec["end_pos"] += by
    return rec, want[1]


def _letters():
    """(targets, budgets, text) as bytes: targets of the LENGTHS over a-y with k = 3 and the TIES with k = 1; the text
    is noise with, per long target, copies with 0 to 4 substituted letters, and begins with the end of target 0 and
    ends with the beginning of target 1, so that seeds point in front of the buffer and behind it"""
    rng = np.random.default_rng(1975)
    ay = np.frombuffer(b"abcdefghijklmnopqrstuvwxy", np.uint8)
    targets = [bytes(rng.choice(ay, size=n)) for n in LENGTHS] + TIES
    ks = [3] * len(LENGTHS) + [1] * len(TIES)
    parts = [targets[0][-9:]]
    for t in targets[:len(LENGTHS)]:
        for d in (0, 1, 2, 3, 4):
            copy = bytearray(t)
            for at in rng.choice(len(t), size=d, replace=False):
                copy[at] = ord("z")                                  # (no target holds a z at these places)
            parts += [bytes(rng.choice(ay, size=int(rng.integers(3, 40)))), bytes(copy)]
    parts += [b" zabcdefgh abcdefgx abcdefgy xbcdefgh zabcdefxh ", bytes(rng.choice(ay, size=200)), targets[1][:9]]
    return targets, ks, b"".join(parts)


@functools.lru_cache(maxsize=None)
def _main(sb):
    """(targets, budgets, text, the plain-Python cut, tests/brute.py's records, APPROX of them) in symbols of sb bytes;
    in wider symbols one letter of an exact copy of target 1 loses its high byte: a mismatch no low-byte compare sees.
    The two derivations must agree before anything else is compared."""
    t8, ks, text8 = _letters()
    targets = [_sym(t, sb) for t in t8]
    text = _sym(text8, sb)
    if sb > 1:
        at = text8.index(t8[1])
        text[at + 5] ^= DTYPE[sb](HIGH[sb])
    kws, terms = compile_targets(targets, ks)
    rec = brute(kws, text)
    want = approx(rec, text, targets, ks, terms)
    same(want, hamming_scan(text, targets, ks), "the two derivations")
    return targets, ks, text, (kws, terms), rec, want


def _machine(sb, targets, ks, cut):
    m = acm.Machine(sb)
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    kws, terms = cut
    assert [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws and aset.terms.tolist() == [list(t) for p in terms for t in p]
    return m, aset


def test_the_case_is_not_trivial():
    targets, ks, text, (kws, terms), rec, want = _main(1)
    w, d = want[0]["keyword_id"], want[1]
    print("symbols %d, keywords %d, records %d, matches %d, distances %s" % (text.size, len(kws), rec.size, w.size, np.bincount(d).tolist()))
    assert 2000 < text.size < 8192
    for t in range(len(targets)):
        assert np.any(d[w == t] == 0) and np.any(d[w == t] >= 1), t
        assert np.all(d[w == t] <= ks[t])
    S = want[0]["end_pos"].astype(np.int64) + 1 - want[0]["length"].astype(np.int64)
    n_seeds = np.array([seeds_of(rec, targets, terms, int(S[j]), int(w[j])) for j in range(w.size)])
    assert np.count_nonzero(n_seeds > 1) >= 2 and np.all(n_seeds >= 1)
    exact = np.nonzero(d == 0)[0]
    assert all(n_seeds[j] == ks[w[j]] + 1 for j in exact)                         # an exact occurrence: every piece seeds it, one output
    ends, counts = np.unique(want[0]["end_pos"], return_counts=True)
    tie = want[0][want[0]["end_pos"] == ends[np.argmax(counts)]]
    assert [(int(r["length"]), int(r["keyword_id"])) for r in tie] == [(9, 9), (8, 7), (8, 8)]   # length descending, then target id


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_targets_on_every_symbol_size(torch_cuda, sb):
    targets, ks, text, cut, rec, want = _main(sb)
    m, aset = _machine(sb, targets, ks, cut)
    plan = m.plan(0)
    dev = _dev(torch_cuda, text)
    A = plan.approx_create(aset)
    info = A.info()
    assert info["targets"] == len(targets) and info["terms"] == aset.terms.shape[0] == 7 * 4 + 3 * 2 and info["longest"] == 300
    assert info["max_k"] == 3 and info["seed_keywords"] == len(cut[0]) and info["max_postings"] >= 2     # `abcd` is a piece of three targets
    got, n, found = _scan(plan, dev, A, rec.size)
    assert found == rec.size and n == want[0].size
    same(got, want, sb)
    # the join alone on tests/brute.py's records, with the compiled set and with a set compiled for the call
    same(_join(plan, rec, A, dev)[0], want, sb)
    same(_join(plan, rec, aset, dev)[0], want, sb)
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
    same(plan.scan_approx_host(text, aset), want, sb)
    same(plan.scan_approx_host(text, aset, pos_base=5000), _moved(want, 5000), sb)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_approx_host(text, aset, out_capacity=want[0].size - 1)
    assert e.value.code == E_OVERFLOW
    same(m.scan_approx(text, aset), want, sb)
    assert m.scan_path == PATH_GPU
    with pytest.raises(acm.ACMError) as e:
        m.scan_approx(text, aset, out_capacity=want[0].size - 1)
    assert e.value.code == E_OVERFLOW
    wrong = binding.ApproxSet([targets[7]], [1], [[(0, 0, 4), (1, 4, 4)]], sym_size=sb)   # keywords 0 and 1 are pieces of target 0
    with pytest.raises(acm.ACMError) as e:
        m.scan_approx(text, wrong)
    assert e.value.code == E_ARG                                                  # the machine's call knows the spellings
    assert plan.scan_approx_host(text, wrong)[0].size == 0                        # the plan's call cannot: no such seed verifies
    # an empty text, a text without a record
    assert plan.scan_approx_host(np.zeros(0, DTYPE[sb]), aset)[0].size == 0
    got, n, found = _scan(plan, _dev(torch_cuda, _sym(b"q" * 3000, sb)), A, 16)
    assert (n, found) == (0, 0)
    A.close()
    plan.status()


@pytest.mark.parametrize("name", ["dense", "gram", "starts"])
def test_scan_approx_on_plan_kinds(torch_cuda, monkeypatch, kat, name):
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    sb = m.sym_size
    rng = np.random.default_rng(75)
    body = text[:4096].astype(DTYPE[sb])
    targets = [body[100:120].copy(), body[1000:1033].copy(), body[2000:2007].copy()]
    ks = [2, 3, 1]
    stranger = DTYPE[sb](250 if sb == 1 else 0xFFFFF0)                           # (in no target)
    planted = []
    for t, k in zip(targets, ks):
        for d in range(k + 2):
            copy = t.copy()
            copy[rng.choice(t.size, size=d, replace=False)] = stranger
            planted += [copy, body[3000:3011]]
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
    want = approx(rec, buf, targets, ks, terms)
    same(want, hamming_scan(buf, targets, ks), "the two derivations")
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
    buf[1500:1517] = targets[0]
    buf[[1501, 1507, 1516]] = np.uint64(12345)
    before = m.nb_keywords
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    for i in range(before, m.nb_keywords):
        o.add_keyword(np.array(m.keyword(i)[0], np.uint64))
    terms = [[tuple(int(x) for x in t) for t in aset.terms]]
    plan = make_plan(0)
    rec = o.scan(buf)
    want = approx(rec, buf, targets, ks, terms)
    same(want, hamming_scan(buf, targets, ks), "the two derivations")
    assert want[1].tolist() == [0, 1]
    got, n, found = _scan(plan, _dev(torch_cuda, buf), aset, rec.size)
    assert found == rec.size
    same(got, want)
    plan.status()
    mc, _, _, make_classes, _, _ = kind("classes", monkeypatch, kat)
    classes = make_classes(0)
    with pytest.raises(acm.ACMError) as e:
        classes.approx_create(binding.ApproxSet([b"dalloway"], [0], [[(5, 0, 8)]]))
    assert e.value.code == E_INELIGIBLE                                           # verification is bitwise on the caller's text
    # a set made for another plan's symbols: the calls that would be refused need no scratch
    A, L = plan.approx_create(aset), acm.lib()
    assert L.acm_gpu_approx_tmp_bytes(plan.h, A.h, 64, 64, 0) > 0 and L.acm_gpu_scan_approx_tmp_bytes(plan.h, A.h, 64, 64, 64, 0) > 0
    assert L.acm_gpu_approx_tmp_bytes(classes.h, A.h, 64, 64, 0) == 0 and L.acm_gpu_scan_approx_tmp_bytes(classes.h, A.h, 64, 64, 64, 0) == 0
    one = torch_cuda.zeros(64, dtype=torch_cuda.int64, device="cuda")
    assert L.acm_gpu_scan_approx_device(classes.h, A.h, one.data_ptr(), 8, 0, None, 0, 4, one.data_ptr(), None, 1, one.data_ptr(), one.data_ptr() + 8,
                                        one.data_ptr(), 512, None) == E_ARG
    A.close()


def test_text_boundaries_of_a_packed_batch(torch_cuda):
    targets, ks, text, cut, rec, want = _main(1)
    kws, terms = cut
    t8 = bytes(text)
    inside = t8.index(bytes(targets[3])) + 11                                    # a cut inside the exact copy of target 3
    at_end = t8.index(bytes(targets[4])) + 32                                    # a text that ends with the exact copy of target 4
    off = np.array(sorted([0, 0, 9, inside, at_end, at_end, 3000, text.size, text.size]), np.uint64)
    cut_want = approx(rec, text, targets, ks, terms, off)
    same(cut_want, hamming_scan(text, targets, ks, off), "the two derivations")
    whole = {tuple(int(x) for x in r) for r in want[0]}
    kept = {tuple(int(x) for x in r) for r in cut_want[0]}
    assert (inside - 11 + 30, 31, 3) in whole - kept and (at_end - 1, 32, 4) in kept and 0 < len(kept) < len(whole)
    # the seeds at the buffer's two ends: `targets[0][-9:]` holds the third piece of target 0 from its second symbol on, whose target
    # would begin in front of the buffer, `targets[1][:9]` the first piece of target 1, whose target would end behind it
    first, last = terms[0][2], terms[1][0]
    assert (1 + first[2] - 1, first[2], first[0]) in {tuple(int(x) for x in r) for r in rec[:4]}
    assert (text.size - 9 + last[2] - 1, last[2], last[0]) in {tuple(int(x) for x in r) for r in rec[-8:]}
    m, aset = _machine(1, targets, ks, cut)
    plan = m.plan(0)
    dev, d_off = _dev(torch_cuda, text), _dev(torch_cuda, off.astype(np.int64))
    same(_join(plan, rec, aset, dev, offsets=d_off)[0], cut_want)
    same(_join(plan, rec, aset, dev)[0], want)
    got, n, found = _scan(plan, dev, aset, rec.size, offsets=d_off)
    assert found == rec.size
    same(got, cut_want)
    same(plan.scan_approx_host(text, aset, offsets=off), cut_want)
    same(m.scan_approx(text, aset, offsets=off), cut_want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_approx_host(text, aset, offsets=[0, 9, 5, text.size])
    assert e.value.code == E_ARG
    plan.status()                                                                 # a seed that points outside its text is no error


def test_more_records_than_the_grid_has_groups(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles"""
    monkeypatch.setenv("ACM_GPU_APPROX_TILE", "64")
    targets, ks = [b"abbab", b"babab", b"aab"], [1, 1, 0]
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = ((8 * cus + 3) * 64 + 65) * 3 // 2                                        # (three records per four symbols)
    text = bytes(np.random.default_rng(8).choice(np.frombuffer(b"ab", np.uint8), size=n))
    m = acm.Machine(1)
    aset = binding.ApproxSet.from_targets(m, targets, ks)
    kws, terms = compile_targets(targets, ks)
    rec = oracle_records([bytes(kw) for kw in kws], text)
    assert rec.size > (8 * cus + 2) * 64 + 65
    want = hamming_scan(text, targets, ks)
    head = rec[rec["end_pos"] < 3000]
    part = approx(head, text[:3000], targets, ks, terms)
    same(part, hamming_scan(text[:3000], targets, ks), "the two derivations, where the loop is affordable")
    plan = m.plan(0)
    got, cnt = _join(plan, rec, aset, _dev(torch_cuda, text), out_capacity=want[0].size)
    same(got, want)
    assert n // 4 < want[0].size
    plan.status()


def test_out_capacity_counts_on_the_device_and_overflow(torch_cuda):
    torch = torch_cuda
    targets, ks, text, cut, rec, want = _main(1)
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
        out, dist, cnt = plan.approx_records(d_rec, rec.size if room is None else room, A, dev, out=d_out, dist=d_dist, out_capacity=out_capacity, count=count)
        return _rec_host(d_out, sentinel.size), _dist_host(d_dist, total + 8), int(cnt.item())
    # the exact room; one short: the count is exact and nothing is written at or behind out_capacity; no room: the count alone
    out, dist, n = join(total)
    assert n == total and np.array_equal(out[total:], sentinel[total:]) and np.all(dist[total:] == 0x5A5A)
    same((out[:n], dist[:n]), want)
    out, dist, n = join(total - 1)
    assert n == total and np.array_equal(out[total - 1:], sentinel[total - 1:]) and np.all(dist[total - 1:] == 0x5A5A)
    out, dist, n = join(0)
    assert n == total and np.array_equal(out, sentinel) and np.all(dist == 0x5A5A)
    out, dist, n = join(1)
    assert n == total and np.array_equal(out[1:], sentinel[1:]) and np.all(dist[1:] == 0x5A5A)
    out, dist, n = join(total + 5)                                                # more room than matches: the padding of the order is not seen
    assert n == total and np.array_equal(out[total:], sentinel[total:]) and np.all(dist[total:] == 0x5A5A)
    same((out[:n], dist[:n]), want)
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
    # dist may be NULL
    L = acm.lib()
    d_rec, d_out, cnt = _rec_dev(torch, rec), _rec_dev(torch, sentinel), torch.zeros(1, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_approx_tmp_bytes(plan.h, A.h, rec.size, total, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    assert L.acm_gpu_approx_records_device(plan.h, A.h, d_rec.data_ptr(), rec.size, None, dev.data_ptr(), text.size, 0, None, 0, d_out.data_ptr(), None,
                                           total, cnt.data_ptr(), tmp.data_ptr(), tb, None) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == total and np.array_equal(_rec_host(d_out, total), want[0])
    # refused calls, and what they would need
    assert tb > 0 and L.acm_gpu_approx_tmp_bytes(plan.h, A.h, 1 << 31, 0, 0) == 0 and L.acm_gpu_approx_tmp_bytes(plan.h, A.h, 64, 1 << 31, 0) == 0
    assert L.acm_gpu_approx_tmp_bytes(plan.h, None, 64, 64, 0) == 0 and L.acm_gpu_scan_approx_tmp_bytes(plan.h, A.h, 1 << 31, 64, 64, 0) == 0
    assert L.acm_gpu_scan_approx_tmp_bytes(plan.h, A.h, 64, 64, 64, 0) > 0

    def call(approx_h=A.h, records=d_rec.data_ptr(), n=rec.size, text_ptr=dev.data_ptr(), out=d_out.data_ptr(), cap=total, count=cnt.data_ptr(),
             scratch=tmp.data_ptr(), tmp_bytes=tb):
        return L.acm_gpu_approx_records_device(plan.h, approx_h, records, n, None, text_ptr, text.size, 0, None, 0, out, None, cap, count, scratch, tmp_bytes, None)
    assert call(approx_h=None) == E_ARG and call(records=None) == E_ARG and call(text_ptr=None) == E_ARG and call(out=None) == E_ARG
    assert call(count=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(cap=1 << 31) == E_ARG and call(out=d_rec.data_ptr()) == E_ARG     # d_out overlapping d_records
    A.close()
    plan.status()


def test_approx_device_arguments(torch_cuda):
    torch = torch_cuda
    targets, ks, text, cut, rec, want = _main(1)
    m, aset = _machine(1, targets, ks, cut)
    plan = m.plan(0)
    A = plan.approx_create(aset)
    L = acm.lib()
    dev = _dev(torch, text)
    total = want[0].size
    d_rec = _rec_dev(torch, rec, 2 * rec.size + total)
    sentinel = np.zeros(total, po.RECORD_DTYPE)
    sentinel["end_pos"], sentinel["length"], sentinel["keyword_id"] = SENTINEL, 7, 7
    d_out = _rec_dev(torch, sentinel)
    d_dist = torch.full((total,), 0x5A5A, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 0x5A5A, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_approx_tmp_bytes(plan.h, A.h, rec.size, total, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")

    def call(plan_h=plan.h, approx_h=A.h, records=d_rec.data_ptr(), n=rec.size, out=d_out.data_ptr(), cap=total, cnt=count.data_ptr(),
             scratch=tmp.data_ptr(), tmp_bytes=tb, offsets=None, n_texts=0):
        return L.acm_gpu_approx_records_device(plan_h, approx_h, records, n, None, dev.data_ptr(), text.size, 0, offsets, n_texts, out, d_dist.data_ptr(), cap,
                                               cnt, scratch, tmp_bytes, None)
    assert tb > 0 and total > 0
    assert call(plan_h=None) == E_ARG and call(approx_h=None) == E_ARG and call(records=None) == E_ARG and call(out=None) == E_ARG
    assert call(cnt=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(cap=1 << 31) == E_ARG
    assert call(out=d_rec.data_ptr()) == E_ARG and call(out=d_rec.data_ptr() + 16 * (rec.size - 1)) == E_ARG     # d_out overlapping d_records
    assert call(out=d_rec.data_ptr() - 16 * (total - 1)) == E_ARG
    assert call(offsets=d_rec.data_ptr(), n_texts=0) == E_ARG                     # no text, but symbols
    if torch.cuda.device_count() > 1:                                             # a set of another device
        elsewhere = m.plan(1)
        B = elsewhere.approx_create(aset)
        assert call(approx_h=B.h) == E_ARG
        B.close()
        elsewhere.close()
        torch.cuda.set_device(0)
    torch.cuda.synchronize()
    assert np.array_equal(_rec_host(d_out, total), sentinel) and np.all(_dist_host(d_dist, total) == 0x5A5A) and int(count.item()) == 0x5A5A   # nothing was touched
    assert call(out=d_rec.data_ptr() + 16 * rec.size) == 0                        # right behind the records: no overlap
    torch.cuda.synchronize()
    same((_rec_host(d_rec[rec.size:], int(count.item())), _dist_host(d_dist, total)), want)
    assert call() == 0
    torch.cuda.synchronize()
    same((_rec_host(d_out, int(count.item())), _dist_host(d_dist, total)), want)
    assert call(n=0, records=None, scratch=None, tmp_bytes=0) == 0                # no record: no match
    torch.cuda.synchronize()
    assert int(count.item()) == 0
    A.close()
    plan.status()


def test_offsets_that_break_the_contract_match_nothing(torch_cuda):
    torch = torch_cuda
    targets, ks, text, cut, rec, want = _main(1)
    m, aset = _machine(1, targets, ks, cut)
    n = text.size
    sentinel = np.zeros(want[0].size, po.RECORD_DTYPE)
    sentinel["end_pos"] = SENTINEL
    dev = _dev(torch, text)
    for what, off in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]), ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n]), *broken_last_pair(n)):
        plan = m.plan(0)
        plan.status()
        d_out = _rec_dev(torch, sentinel)
        out, dist, cnt = plan.approx_records(_rec_dev(torch, rec), rec.size, aset, dev, offsets=_dev(torch, np.array(off, np.int64)), out=d_out)
        assert int(cnt.item()) == 0, what
        assert np.array_equal(_rec_host(d_out, sentinel.size), sentinel), what
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_records_that_break_the_contract_are_skipped_and_reported(torch_cuda):
    targets, ks, text, cut, rec, want = _main(1)
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


def test_a_pending_delta_after_plan_update(torch_cuda):
    targets, ks, text, cut, rec, want = _main(1)
    m = acm.Machine(1)
    early = binding.ApproxSet.from_targets(m, targets[7:8], ks[7:8])              # abcd, efgh
    plan = m.plan(0)
    A0 = plan.approx_create(early)
    aset = binding.ApproxSet.from_targets(m, targets, ks)                         # more pieces: the machine is ahead of the plan
    with pytest.raises(acm.ACMError) as e:
        plan.approx_create(aset)
    assert e.value.code == E_ARG                                                  # the plan does not know them yet
    plan.update(m)
    A = plan.approx_create(aset)
    words = [m.keyword(i)[0] for i in range(m.nb_keywords)]
    terms = [[tuple(int(x) for x in aset.terms[i]) for i in range(int(aset.tgt_ptr[w]), int(aset.tgt_ptr[w + 1]))] for w in range(len(targets))]
    assert words[:2] == [tuple(b"abcd"), tuple(b"efgh")] and terms != cut[1]      # (other ids than the plain cut's: the records are made anew)
    rec2 = brute(words, text)
    same(approx(rec2, text, targets, ks, terms), want, "the same matches under other keyword ids")
    dev = _dev(torch_cuda, text)
    got, n, found = _scan(plan, dev, A, rec2.size)
    assert found == rec2.size
    same(got, want)
    # the set made before the update stays valid
    same(_scan(plan, dev, A0, rec2.size)[0], hamming_scan(text, targets[7:8], ks[7:8]))
    same(m.scan_approx(text, aset), want)
    A.close()
    A0.close()
    plan.status()


def test_six_words_of_the_novel_at_k_1_and_2(torch_cuda, novel_bytes):
    text = novel_bytes[:8192]
    words = [b"Clarissa", b"Dalloway", b"would", b"there", b"then", b"morning"]
    for k in (1, 2):
        ks = [k] * len(words)
        m = acm.Machine(1)
        aset = binding.ApproxSet.from_targets(m, words, k)
        kws, terms = compile_targets(words, ks)
        assert [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws
        want = hamming_scan(text, words, ks)                                      # the numpy brute force
        per = np.bincount(want[0]["keyword_id"], minlength=len(words))
        print("k = %d: matches per word %s, distances %s" % (k, per.tolist(), np.bincount(want[1]).tolist()))
        assert np.all(per >= 2) and np.count_nonzero(want[1]) >= 3 * k
        plan = m.plan(0)
        rec = oracle_records([bytes(kw) for kw in kws], text)
        got, n, found = _scan(plan, _dev(torch_cuda, text), aset, rec.size)
        assert found == rec.size
        same(got, want, k)
        same(m.scan_approx(text, aset), want, k)
        plan.status()
