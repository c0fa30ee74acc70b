"""Anchored matches and the dictionary lookup on the GPU (acm_gpu_scan_anchored_*, acm_gpu_lookup_*,
acm_scan_anchored, acm_lookup; csrc/dev_anchored.h).  The expected answer is always the definition of
ANCHORED and LOOKUP in plain Python over the ORACLE's records (tests/anchored_cases.py), never the
library's own scan or filter; every comparison is bit-exact.  Outputs are pre-filled with a pattern,
so that a missing write and a write too many both show."""
import ctypes as C

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from oracle import pyoracle as po
from tests import anchored_cases as ac
from tests.batch_cases import broken_last_pair
from tests.cases import build_pair
from tests.tally_cases import KINDS, PATH_CLASSES, PATH_GPU, byte_oracle, kind

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
PATTERN, PATTERN32 = 0x0123456789ABCDEF, 0x5A5A5A5A
GUARD = 256


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


def _sym(letters, sb):
    """the letters of a byte string as symbols of sb bytes"""
    return (np.frombuffer(bytes(letters), np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(DTYPE[sb])


def _full(torch, n, dtype, value):
    return torch.full((max(n, 1),), value - (1 << 32) if dtype == torch.int32 and value >= 1 << 31 else value, dtype=dtype, device="cuda")


class Got:
    pass


def _anchored(torch, plan, dev, d_off, mode, capacity, n_symbols=None, short_by=0, guard=False):
    """acm_gpu_scan_anchored_device through binding.lib () on pre-filled outputs with one record, one text id
    of room more than `capacity`; guard: the scratch is exactly *_tmp_bytes between two 256-byte guards of 0xFF"""
    L = binding.lib()
    g = Got()
    n_texts = d_off.numel() - 1
    n_symbols = dev.numel() * dev.element_size() // plan.sym_size if n_symbols is None else n_symbols
    rec = _full(torch, 2 * (capacity + 1), torch.int64, PATTERN)
    tid = _full(torch, capacity + 1, torch.int32, PATTERN32)
    first = _full(torch, n_texts + 1, torch.int64, PATTERN)
    cnt = _full(torch, 1, torch.int64, PATTERN)
    tb = L.acm_gpu_scan_anchored_tmp_bytes(plan.h, n_texts)
    assert tb > 0
    tmp = torch.full((tb + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    g.rc = L.acm_gpu_scan_anchored_device(plan.h, dev.data_ptr(), n_symbols, d_off.data_ptr(), n_texts, mode, rec.data_ptr(), tid.data_ptr(),
                                          first.data_ptr(), capacity, cnt.data_ptr(), tmp.data_ptr() + GUARD, tb - short_by, None)
    torch.cuda.synchronize()
    g.count = int(cnt.item())
    g.rec = np.frombuffer(rec.cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE).copy()
    g.tid = tid.cpu().numpy().view(np.uint32).copy()
    g.first = first.cpu().numpy().view(np.uint64).copy()
    if guard:
        t = tmp.cpu().numpy()
        assert np.all(t[:GUARD] == 0xFF) and np.all(t[GUARD + tb:] == 0xFF), "a guard of the scratch was written"
    return g


def _untouched(g, from_record=0, first=True, count=True):
    ok = np.all(g.rec.view(np.uint64).reshape(-1, 2)[from_record:] == PATTERN) and np.all(g.tid[from_record:] == PATTERN32)
    return ok and (not first or np.all(g.first == PATTERN)) and (not count or g.count == PATTERN)


def _check(g, want, what=None):
    rec, tid, first = want
    n = rec.size
    assert g.rc == 0 and g.count == n, (what, g.rc, g.count, n)
    assert np.array_equal(g.rec[:n], rec), (what, g.rec[:8], rec[:8])
    assert np.array_equal(g.tid[:n], tid) and np.array_equal(g.first, first), what
    assert _untouched(g, from_record=n, first=False, count=False), what


def _lookup(torch, plan, dev, d_off, which=(True, True, True), n_symbols=None, short_by=0, guard=False):
    L = binding.lib()
    n_texts = d_off.numel() - 1
    n_symbols = dev.numel() * dev.element_size() // plan.sym_size if n_symbols is None else n_symbols
    outs = [_full(torch, n_texts + 1, torch.int32, PATTERN32) for _ in range(3)]
    tb = L.acm_gpu_lookup_tmp_bytes(plan.h, n_texts)
    assert tb > 0
    tmp = torch.full((tb + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = L.acm_gpu_lookup_device(plan.h, dev.data_ptr(), n_symbols, d_off.data_ptr(), n_texts, *[o.data_ptr() if w else None for o, w in zip(outs, which)],
                                 tmp.data_ptr() + GUARD, tb - short_by, None)
    torch.cuda.synchronize()
    if guard:
        t = tmp.cpu().numpy()
        assert np.all(t[:GUARD] == 0xFF) and np.all(t[GUARD + tb:] == 0xFF), "a guard of the scratch was written"
    return rc, [o.cpu().numpy().view(np.uint32).copy() for o in outs]


def _check_lookup(got, look, which=(True, True, True), what=None):
    rc, outs = got
    assert rc == 0, what
    for o, w, on in zip(outs, look, which):
        assert o[-1] == PATTERN32, what                          # the entry behind the last text
        assert np.array_equal(o[:-1], w) if on else np.all(o == PATTERN32), what


def _check_everything(torch, plan, dev, d_off, want, look, what=None):
    """all three modes with room for exactly the records, and the lookup arrays"""
    for mode in ac.MODES:
        _check(_anchored(torch, plan, dev, d_off, mode, want[mode][0].size), want[mode], (what, mode))
    _check_lookup(_lookup(torch, plan, dev, d_off), look, what=what)
    plan.status()


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_hand_made_batch_on_every_symbol_size(torch_cuda, sb):
    torch = torch_cuda
    packed, off, want, look = ac.hand_made(byte_oracle(ac.KEYWORDS))
    m, _ = build_pair([_sym(k, sb) for k in ac.KEYWORDS], sb)
    plan = m.plan(0)
    dev, d_off = _dev(torch, _sym(packed, sb)), _dev(torch, off.astype(np.int64))
    _check_everything(torch, plan, dev, d_off, want, look, sb)
    for which in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        _check_lookup(_lookup(torch, plan, dev, d_off, which), look, which, (sb, which))
    # the Python layer: Plan.scan_anchored / Plan.lookup on the device, the host calls, the machine's calls
    for name, mode in (("prefixes", ac.PREFIXES), ("longest", ac.LONGEST), ("whole", ac.WHOLE)):
        rec, tid, first, cnt, _ = plan.scan_anchored(dev, d_off, mode=name, capacity=ac.N_PREFIXES)
        n = int(cnt.item())
        got = np.frombuffer(rec[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE)
        assert np.array_equal(got, want[mode][0]) and np.array_equal(tid[:n].cpu().numpy().view(np.uint32), want[mode][1])
        assert np.array_equal(first.cpu().numpy().view(np.uint64), want[mode][2])
        for got3 in (plan.scan_anchored_host(_sym(packed, sb), off, mode=name), m.scan_anchored([_sym(t, sb) for t in ac.TEXTS], mode=name)):
            assert all(np.array_equal(g, w) for g, w in zip(got3, want[mode])), (sb, name)
    got3 = plan.lookup(dev, d_off)
    assert all(np.array_equal(g.cpu().numpy().view(np.uint32), w) for g, w in zip(got3, look))
    whole_only = plan.lookup(dev, d_off, prefix_id=False, prefix_len=False)
    assert whole_only[1] is None and whole_only[2] is None and np.array_equal(whole_only[0].cpu().numpy().view(np.uint32), look[0])
    for got3 in (plan.lookup_host(_sym(packed, sb), off), m.lookup([_sym(t, sb) for t in ac.TEXTS])):
        assert all(np.array_equal(g, w) for g, w in zip(got3, look)), sb
    assert m.scan_path == PATH_GPU
    plan.status()


@pytest.mark.parametrize("name", KINDS)
def test_every_plan_kind(torch_cuda, monkeypatch, kat, novel_bytes, name):
    """dense, 4-gram, CSR (a dense plan on a pointer one symbol off the 16-byte grid), start-parallel (also
    after an update in place), sparse walk, interned 8-byte symbols, comparator classes (a text whose case
    differs from the dictionary's), a plan with a pending delta: the cut maker's batch of a 1 Mi-symbol text"""
    torch = torch_cuda
    m, o, text, make_plan, plan_ok, form = kind(name, monkeypatch, kat)
    if text is None:
        text = np.frombuffer(novel_bytes, np.uint8)
    text = np.ascontiguousarray(text)
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()
    sb = plan.sym_size
    must = ()
    if name == "starts":
        # a keyword the plan learns by an edit of its tables: five symbols of the text that are no keyword yet
        before = o.nb_keywords
        fresh = text[4321:4326].copy()
        m.add_keyword(fresh)
        o.add_keyword(fresh)
        assert o.nb_keywords == before + 1
        plan.update(m)
        assert plan_ok(plan) and plan.info.delta_keywords == 0 and plan.info.merges == 0, plan.describe()
        must = (before,)
    if name != "classes":                                    # the synthetic texts hold one planted keyword per 4,096 symbols: more of them
        text = ac.plant(text, o.scan(text))
    rec = o.scan(text)
    if name == "delta":
        base, late = rec["keyword_id"][rec["keyword_id"] < 300], rec["keyword_id"][(rec["keyword_id"] >= 300)]
        assert base.size and late.size
        must = (int(base[0]), int(late[0]))
    small = text.size < (1 << 20)
    off, chosen = ac.make_cuts(text.size, rec, n_chosen=1400 if small else 3000, n_random=2000 if small else 3000, must=must)
    want, look = ac.expected(o, text, off)
    ac.nontrivial(want, look, chosen)
    for k in must:                                           # from the oracle: a chosen record of each, hence an anchored one
        assert np.any(chosen["keyword_id"] == k) and np.any(want[ac.PREFIXES][0]["keyword_id"] == k), k
    if name == "classes":                                    # the dictionary says He / SHE / hErs / Mrs / dalloway: the novel spells none of them so
        spelled = {bytes(text[int(r["end_pos"]) + 1 - int(r["length"]):int(r["end_pos"]) + 1]) for r in want[ac.PREFIXES][0][:400]}
        assert len(spelled - {b"He", b"SHE", b"his", b"hErs", b"Mrs", b"dalloway", b"Zyzzyva"}) >= 3, spelled
    if name == "csr":
        whole = _dev(torch, np.concatenate([np.zeros(16 + sb, text.dtype), text]))
        dev = whole[(16 + sb) // sb:]
        assert whole.data_ptr() % 16 == 0 and dev.data_ptr() % 16 == sb and dev.is_contiguous()
    else:
        dev = _dev(torch, text)
    d_off = _dev(torch, off.astype(np.int64))
    _check_everything(torch, plan, dev, d_off, want, look, name)
    assert plan_ok(plan)


def test_grid_stride_and_text_counts(torch_cuda, monkeypatch, novel_bytes):
    torch = torch_cuda
    keywords, o, text, off, want, look = ac.novel_batch(novel_bytes, n_chosen=2000, n_random=2500)
    assert off.size - 1 >= 5000
    m, _ = build_pair(keywords, 1)
    plan = m.plan(0)
    dev, d_off = _dev(torch, text), _dev(torch, off.astype(np.int64))
    _check_everything(torch, plan, dev, d_off, want, look, "full grid")
    monkeypatch.setenv("ACM_GPU_ANCHORED_GRID", "3")            # three blocks of 256 lanes stride over 5,000 texts and more
    _check_everything(torch, plan, dev, d_off, want, look, "three blocks")
    monkeypatch.setenv("ACM_GPU_ANCHORED_GRID", "1")
    _check_everything(torch, plan, dev, d_off, want, look, "one block")
    monkeypatch.delenv("ACM_GPU_ANCHORED_GRID")
    # 1, 63, 64, 65 texts: the first texts of the batch, the buffer cut where the last of them ends
    for n_texts in (1, 63, 64, 65, 257):
        part_off = off[:n_texts + 1]
        n_sym = int(part_off[-1])
        w, l = ac.expected(o, text[:n_sym], part_off)
        _check_everything(torch, plan, dev[:n_sym], _dev(torch, part_off.astype(np.int64)), w, l, n_texts)
    # no text: no symbol, a zero in the count and in first[0], nothing else
    zero = _dev(torch, np.zeros(1, np.int64))
    g = _anchored(torch, plan, dev, zero, ac.PREFIXES, 4, n_symbols=0)
    assert g.rc == 0 and g.count == 0 and g.first.tolist() == [0] and _untouched(g, first=False, count=False)
    assert _anchored(torch, plan, dev, zero, ac.PREFIXES, 4, n_symbols=5).rc == E_ARG
    rc, outs = _lookup(torch, plan, dev, zero, n_symbols=0)
    assert rc == 0 and all(np.all(o_ == PATTERN32) for o_ in outs)
    plan.status()


def test_text_lengths_around_lmax(torch_cuda):
    """a text longer than lmax whose first lmax symbols spell a keyword, one of exactly lmax, one a symbol
    shorter than a keyword it is a prefix of -- behind an aligned pointer and one symbol past it"""
    torch = torch_cuda
    keywords = [b"ab", b"abcdefgh", b"abcd", b"b"]                   # lmax = 8
    texts = [b"abcdefghij", b"abcdefgh", b"abcdefg", b"abcdefghabcdefgh", b"abc", b"a", b"b", b"", b"abcdefgX"]
    o = byte_oracle(keywords)
    from tests.batch_cases import offsets_of, oracle_batch
    off = offsets_of(texts)
    rec, tid, _ = oracle_batch(o, texts)
    want = {mode: ac.anchored(rec, off, mode, tid) for mode in ac.MODES}
    look = ac.lookup(rec, off, tid)
    assert np.diff(want[ac.PREFIXES][2].astype(np.int64)).tolist() == [3, 3, 2, 3, 1, 0, 1, 0, 2]
    assert look[0].tolist() == [ac.NONE, 1, ac.NONE, ac.NONE, ac.NONE, ac.NONE, 3, ac.NONE, ac.NONE] and look[2].tolist() == [8, 8, 4, 8, 2, 0, 1, 0, 4]
    m, _ = build_pair(keywords, 1)
    plan = m.plan(0)
    packed = np.frombuffer(b"".join(texts), np.uint8)
    d_off = _dev(torch, off.astype(np.int64))
    for lead in (16, 1):
        whole = _dev(torch, np.concatenate([np.full(lead, ord("a"), np.uint8), packed]))    # (nothing behind the last text: it ends the allocation's data)
        dev = whole[lead:]
        assert dev.data_ptr() % 16 == lead % 16
        _check_everything(torch, plan, dev, d_off, want, look, lead)


def test_capacity_holds_the_anchored_records_only(torch_cuda, novel_bytes):
    torch = torch_cuda
    keywords, o, text, off, want, look = ac.novel_batch(novel_bytes)
    m, _ = build_pair(keywords, 1)
    plan = m.plan(0)
    dev, d_off = _dev(torch, text), _dev(torch, off.astype(np.int64))
    n, n_texts = want[ac.PREFIXES][0].size, off.size - 1
    assert n < o.scan(text).size // 4                                 # far fewer than the matches of the buffer
    _check(_anchored(torch, plan, dev, d_off, ac.PREFIXES, n), want[ac.PREFIXES], "exactly the count")
    g = _anchored(torch, plan, dev, d_off, ac.PREFIXES, n - 1)
    assert g.rc == 0 and g.count == n and np.array_equal(g.first, want[ac.PREFIXES][2])   # the need, and first[] complete
    assert _untouched(g, from_record=n - 1, first=False, count=False)                     # the guard record behind d_records[capacity)
    g = _anchored(torch, plan, dev, d_off, ac.PREFIXES, 0)
    assert g.rc == 0 and g.count == n and np.array_equal(g.first, want[ac.PREFIXES][2]) and _untouched(g, first=False, count=False)
    for mode in (ac.LONGEST, ac.WHOLE):                                                   # capacity = n_texts never overflows
        g = _anchored(torch, plan, dev, d_off, mode, n_texts)
        assert want[mode][0].size <= n_texts
        _check(g, want[mode], mode)
    # the host call says so with its return value and the need; the Python wrapper repeats the call once
    out = np.zeros(4, po.RECORD_DTYPE)
    nf = C.c_uint64(0)
    tid4, first = np.full(4, PATTERN32, np.uint32), np.full(n_texts + 1, PATTERN, np.uint64)
    rc = binding.lib().acm_gpu_scan_anchored_host(plan.h, text, off.ctypes.data, n_texts, ac.PREFIXES, out.ctypes.data, tid4.ctypes.data,
                                                  first.ctypes.data, 4, C.byref(nf))
    assert rc == E_OVERFLOW and nf.value == n
    assert np.array_equal(first, want[ac.PREFIXES][2]) and np.all(tid4 == PATTERN32) and not out.view(np.uint64).any()   # first[] complete, no record
    got3 = plan.scan_anchored_host(np.frombuffer(text, np.uint8), off)
    assert all(np.array_equal(g_, w) for g_, w in zip(got3, want[ac.PREFIXES]))
    plan.status()


def test_offsets_that_break_the_contract_write_nothing(torch_cuda):
    torch = torch_cuda
    packed, off, want, look = ac.hand_made(byte_oracle(ac.KEYWORDS))
    m, _ = build_pair(ac.KEYWORDS, 1)
    dev = _dev(torch, packed)
    cases = {"first": off.copy(), "last": off.copy(), "decrease": off.copy()}
    cases["first"][0] = 1
    cases["last"][-1] -= 1
    cases["decrease"][6], cases["decrease"][7] = off[7] + 3, off[6]
    assert cases["decrease"][6] > cases["decrease"][7]
    cases.update((what, np.array(bad, off.dtype)) for what, bad in broken_last_pair(len(packed)))
    for what, bad in cases.items():
        d_bad = _dev(torch, bad.astype(np.int64))
        plan = m.plan(0)
        g = _anchored(torch, plan, dev, d_bad, ac.PREFIXES, ac.N_PREFIXES)
        assert g.rc == 0 and g.count == 0 and _untouched(g, count=False), what
        with pytest.raises(binding.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan = m.plan(0)
        rc, outs = _lookup(torch, plan, dev, d_bad)
        assert rc == 0 and all(np.all(o_ == PATTERN32) for o_ in outs), what
        with pytest.raises(binding.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        if what in ("first", "decrease"):   # (the host calls have no n_symbols argument: there the last offset IS the number of symbols)
            nf = C.c_uint64(0)
            L = binding.lib()
            assert L.acm_gpu_scan_anchored_host(plan.h, packed, bad.ctypes.data, bad.size - 1, 1, None, None, None, 0, C.byref(nf)) == E_ARG
            w = np.zeros(bad.size, np.uint32)
            assert L.acm_gpu_lookup_host(plan.h, packed, bad.ctypes.data, bad.size - 1, w.ctypes.data, None, None) == E_ARG
        # afterwards the same plan still answers a good batch, and scans (its status stays raised: a fresh plan reports clean)
        d_off = _dev(torch, off.astype(np.int64))
        _check(_anchored(torch, plan, dev, d_off, ac.PREFIXES, ac.N_PREFIXES), want[ac.PREFIXES], what)
        _check_lookup(_lookup(torch, plan, dev, d_off), look, what=what)
        assert np.array_equal(plan.scan_host(np.frombuffer(packed, np.uint8)), byte_oracle(ac.KEYWORDS).scan(packed))
    plan = m.plan(0)
    _check_everything(torch, plan, dev, _dev(torch, off.astype(np.int64)), want, look, "a fresh plan")


def test_scratch_is_what_tmp_bytes_reports_and_the_other_argument_checks(torch_cuda, novel_bytes):
    """exactly *_tmp_bytes between two 256-byte guards of 0xFF: the same answers, the guards untouched;
    one byte less: ACM_GPU_E_ARG and no output touched (tests/test_scratch_bounds_gpu.py's rule)"""
    torch = torch_cuda
    keywords, o, text, off, want, look = ac.novel_batch(novel_bytes)
    m, _ = build_pair(keywords, 1)
    plan = m.plan(0)
    dev, d_off = _dev(torch, text), _dev(torch, off.astype(np.int64))
    for mode in ac.MODES:
        _check(_anchored(torch, plan, dev, d_off, mode, want[mode][0].size, guard=True), want[mode], mode)
        g = _anchored(torch, plan, dev, d_off, mode, want[mode][0].size, short_by=1, guard=True)
        assert g.rc == E_ARG and _untouched(g), mode
    _check_lookup(_lookup(torch, plan, dev, d_off, guard=True), look)
    rc, outs = _lookup(torch, plan, dev, d_off, short_by=1, guard=True)
    assert rc == E_ARG and all(np.all(o_ == PATTERN32) for o_ in outs)
    # the other refusals, none of which touches an output
    n_texts = off.size - 1
    for mode in (0, 4):
        g = _anchored(torch, plan, dev, d_off, mode, n_texts)
        assert g.rc == E_ARG and _untouched(g)
    rc, outs = _lookup(torch, plan, dev, d_off, which=(False, False, False))
    assert rc == E_ARG
    L = binding.lib()
    cnt = _full(torch, 1, torch.int64, PATTERN)                     # too many texts: refused before anything is sized by them
    assert L.acm_gpu_scan_anchored_device(plan.h, dev.data_ptr(), dev.numel(), d_off.data_ptr(), (1 << 31) - 1, ac.PREFIXES, None, None, None, 0, cnt.data_ptr(),
                                          dev.data_ptr(), 1 << 18, None) == E_ARG
    assert L.acm_gpu_lookup_device(plan.h, dev.data_ptr(), dev.numel(), d_off.data_ptr(), 1 << 32, cnt.data_ptr(), None, None, dev.data_ptr(), 1 << 18,
                                   None) == E_ARG
    torch.cuda.synchronize()
    assert int(cnt.item()) == PATTERN
    assert L.acm_gpu_scan_anchored_tmp_bytes(plan.h, (1 << 31) - 1) == 0 and L.acm_gpu_lookup_tmp_bytes(plan.h, 1 << 32) == 0      # n_texts + 1 items in 31 bits
    assert L.acm_gpu_scan_anchored_tmp_bytes(plan.h, (1 << 31) - 2) > 0 and L.acm_gpu_lookup_tmp_bytes(plan.h, (1 << 32) - 1) > 0
    plan.status()


def test_machine_calls_on_a_gpu_machine_and_a_classes_machine(torch_cuda, monkeypatch, kat, novel_bytes):
    """acm_scan_anchored and acm_lookup through the cached plan: the plain GPU path, also after the
    machine grew (acm_gpu_plan_update), and the path over comparator classes"""
    keywords, o, text, off, want, look = ac.novel_batch(novel_bytes)
    texts = [text[int(off[t]):int(off[t + 1])] for t in range(off.size - 1)]
    m, _ = build_pair(keywords[:-40], 1)
    m.scan_anchored(texts[:50])                                  # the cached plan is made from the shorter dictionary
    for kw in keywords[-40:]:
        m.add_keyword(kw)
    for name, mode in (("prefixes", ac.PREFIXES), ("longest", ac.LONGEST), ("whole", ac.WHOLE)):
        got3 = m.scan_anchored(texts, mode=name)
        assert all(np.array_equal(g, w) for g, w in zip(got3, want[mode])), name
    assert all(np.array_equal(g, w) for g, w in zip(m.lookup(texts), look))
    assert m.scan_path == PATH_GPU
    with pytest.raises(acm.ACMError) as e:
        m.scan_anchored(texts, capacity=want[ac.PREFIXES][0].size - 1)
    assert e.value.code == E_OVERFLOW and m.scan_path == PATH_GPU
    # comparator classes: the novel under a dictionary in another case
    mc, oc, _, make_plan, plan_ok, form = kind("classes", monkeypatch, kat)
    part = novel_bytes[:150000]
    offc, chosen = ac.make_cuts(len(part), oc.scan(part), n_chosen=1200, n_random=1200)
    wantc, lookc = ac.expected(oc, part, offc)
    ac.nontrivial(wantc, lookc, chosen, many=False)
    textsc = [part[int(offc[t]):int(offc[t + 1])] for t in range(offc.size - 1)]
    for name, mode in (("prefixes", ac.PREFIXES), ("longest", ac.LONGEST), ("whole", ac.WHOLE)):
        got3 = mc.scan_anchored(textsc, mode=name)
        assert all(np.array_equal(g, w) for g, w in zip(got3, wantc[mode])), name
    assert all(np.array_equal(g, w) for g, w in zip(mc.lookup(textsc), lookc))
    assert mc.scan_path == PATH_CLASSES


def test_split_lines_go_straight_into_the_lookup(torch_cuda, novel_bytes):
    """acm_gpu_split_device's offsets never visit the host: lines of the novel into acm_gpu_lookup_device"""
    torch = torch_cuda
    from tests.tally_cases import novel_words
    part = novel_bytes[:100000]
    line = [ln for ln in part.splitlines(keepends=True) if len(ln) > 40][7]    # a whole line, its newline included, as one more keyword
    keywords = novel_words(novel_bytes) + [line]
    o = byte_oracle(keywords)
    m, _ = build_pair(keywords, 1)
    plan = m.plan(0)
    dev = _dev(torch, part)
    d_off = plan.split(dev, delims=b"\n")
    rc, outs = _lookup(torch, plan, dev, d_off)
    off = d_off.cpu().numpy().view(np.uint64)
    want, look = ac.expected(o, part, off)
    assert np.count_nonzero(look[1] != ac.NONE) >= 200 and np.count_nonzero(look[0] != ac.NONE) >= 1, "lines that begin with a word of the novel"
    _check_lookup((rc, outs), look)
    _check(_anchored(torch, plan, dev, d_off, ac.PREFIXES, want[ac.PREFIXES][0].size), want[ac.PREFIXES])
    plan.status()
