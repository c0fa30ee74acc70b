"""Keyword templates with symbol classes on the GPU (acm_gpu_templates_*, acm_gpu_scan_templates_*,
acm_scan_templates; csrc/dev_templates.h).  The expected answer is always the definition of TEMPLATES in plain Python
over the ORACLE's or tests/brute.py's records (tests/template_cases.py) and, the cuts being canonical, a second
derivation from the text alone (a numpy acceptance matrix per template) -- never the library's own scan or pass.  All
comparisons are exact, order and distances included.  Texts are a few KiB; one case has more records than the capped
grid has groups of tiles of 64, so that blocks stride over tiles.  The bitmaps of byte classes are read from global
memory: there is no staging limit whose two sides would need a case."""
import functools

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
from aho_corasick_1975_amd import binding
from aho_corasick_1975_amd.binding import ANY, SymbolClass, TemplateSet
from oracle import pyoracle as po
from tests import template_cases as tc
from tests.tally_cases import PATH_GPU, kind
from tests.template_cases import same

pytestmark = pytest.mark.gpu

E_ARG, E_OVERFLOW, E_INELIGIBLE, E_INTERNAL = binding.ACM_GPU_E_ARG, binding.ACM_GPU_E_OVERFLOW, binding.ACM_GPU_E_INELIGIBLE, -7
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
HIGH = {1: 0, 2: 0x4100, 4: 0x41000000, 8: 0x4100000000000000}   # set in every wider symbol: a compare of the low byte alone is seen
SENTINEL = 0x0123456789ABCDEF
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 300)                         # the rounds of a 16-lane group
Z = ord("z")


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


def _join(plan, rec, templates, dev_text, **kw):
    """Plan.templates_records on the records `rec` (host): ((the matches, their distances) (host), the count)"""
    torch = __import__("torch")
    out, dist, cnt = plan.templates_records(_rec_dev(torch, rec), rec.size, templates, dev_text, **kw)
    n = int(cnt.item())
    return (_rec_host(out, min(n, out.shape[0])), _dist_host(dist, min(n, out.shape[0]))), n


def _scan(plan, dev, templates, capacity, **kw):
    """Plan.scan_templates: ((the matches, their distances) (host), the count, the scan's count)"""
    out, dist, cnt, found, _ = plan.scan_templates(dev, templates, capacity=capacity, **kw)
    n = int(cnt.item())
    return (_rec_host(out, min(n, out.shape[0])), _dist_host(dist, min(n, out.shape[0]))), n, int(found.item())


def _moved(want, by):
    rec = want[0].copy()
    rec["end_pos"] += by
    return rec, want[1]


def _lift(cell, hi):
    """a cell over letters as a cell over symbols with the high byte `hi` set"""
    if cell is ANY:
        return ANY
    if isinstance(cell, SymbolClass):
        return SymbolClass([(lo | hi, up | hi) for lo, up in cell.ranges], cell.negate)
    return int(cell) | hi


def _letters():
    """(templates, budgets, text, failing) over letters.  Per length of LENGTHS one template of random letters a to w with
    class cells at index 0 (the letter and its two neighbours), 15 (everything but q and z), 16 (a range of three) and
    L - 1 (the letter or Z), and ANY at index 5; budget 3, and 0 for the one-cell template and for a second template of
    17 cells.  Three more with budget 1 end at one symbol.  The text is noise a to y with, per long template, copies
    with 0 to 4 failing cells (a z where the cell does not take it; the first failing cell is a class cell in every
    other copy), begins with the end of template 1 and ends with the beginning of template 2, so that seeds point in
    front of the buffer and behind it.  failing: (template, the text index of the copy, the failing cells)."""
    rng = np.random.default_rng(1975)
    aw, ay = np.frombuffer(b"abcdefghijklmnopqrstuvw", np.uint8), np.frombuffer(b"abcdefghijklmnopqrstuvwxy", np.uint8)

    def make(L):
        t = [int(x) for x in rng.choice(aw, size=L)]
        if L == 1:
            return t
        cells = list(t)
        cells[0] = SymbolClass([(max(t[0] - 1, 97), t[0] + 1)])
        cells[5] = ANY
        if L > 15:
            cells[15] = SymbolClass([ord("q"), Z], negate=True)
        if L > 16:
            cells[16] = SymbolClass([(t[16] - 1 if t[16] > 97 else 97, t[16] + 1)])
        cells[L - 1] = SymbolClass([t[L - 1], ord("Z")])
        return cells
    tpls = [make(L) for L in LENGTHS]
    ks = [0 if L == 1 else 3 for L in LENGTHS]
    tpls.append(make(17))
    ks.append(0)
    a_h = [ord(c) for c in "abcdefgh"]
    tpls += [a_h[:7] + [SymbolClass([ord("h"), ord("x")])], a_h[:6] + [SymbolClass([ord("g")]), ord("h")],
             [Z] + a_h[:8][:-1] + [SymbolClass([(ord("a"), ord("h"))])]]
    ks += [1, 1, 1]

    def spelled(cells):
        """letters every cell accepts (ANY and the negated class: an `m`)"""
        return bytes(c if tc.is_literal(c) else ord("m") if c is ANY or c.negate else c.ranges[0][1] if len(c.ranges) == 1 and c.ranges[0][0] != c.ranges[0][1]
                     else c.ranges[0][0] for c in cells)
    parts, failing, at = [spelled(tpls[1])[-9:]], [], 9
    for w, cells in enumerate(tpls[:len(LENGTHS) + 1]):
        can_fail = [i for i, c in enumerate(cells) if c is not ANY]
        classes = [i for i in can_fail if not tc.is_literal(cells[i])]
        for d in range(0, min(4, ks[w] + 1) + 1):
            copy = bytearray(spelled(cells))
            where = [int(x) for x in rng.permutation(can_fail)]
            if classes and d % 2:
                first = classes[(d // 2) % len(classes)]
                where = [first] + [i for i in where if i != first]
            for i in where[:d]:
                copy[i] = Z
            noise = bytes(rng.choice(ay, size=int(rng.integers(3, 40))))
            parts += [noise, bytes(copy)]
            failing.append((w, at + len(noise), sorted(where[:d])))
            at += len(noise) + len(copy)
    parts += [b" zabcdefgh abcdefgx abcdefgy xbcdefgh zabcdefxh ", bytes(rng.choice(ay, size=200)), spelled(tpls[2])[:9]]
    return tpls, ks, b"".join(parts), failing


@functools.lru_cache(maxsize=None)
def _main(sb):
    """(templates, budgets, text, the plain-Python cut, tests/brute.py's records, TEMPLATES of them) in symbols of sb
    bytes; in wider symbols the symbol under class cell 15 of the exact copy of template 2 loses its high byte: a
    failing cell no low-byte compare sees.  The two derivations must agree before anything else is compared."""
    t8, ks, text8, failing = _letters()
    tpls = [[_lift(c, HIGH[sb]) for c in t] for t in t8]
    text = (np.frombuffer(text8, np.uint8).astype(np.uint64) | np.uint64(HIGH[sb])).astype(DTYPE[sb])
    if sb > 1:
        at = [a for w, a, cells in failing if w == 2 and not cells][0]
        text[at + 15] ^= DTYPE[sb](HIGH[sb])
    kws, terms = tc.compile_templates(tpls, ks)
    rec = tc.brute(kws, text)
    want = tc.templates(rec, text, tpls, ks, terms)
    same(want, tc.window_scan(text, tpls, ks), "the two derivations")
    return tpls, ks, text, (kws, terms), rec, want


def _machine(sb, tpls, ks, cut):
    m = acm.Machine(sb)
    tset = TemplateSet.from_templates(m, tpls, ks)
    kws, terms = cut
    assert [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws and tset.terms.tolist() == [list(t) for p in terms for t in p]
    return m, tset


def test_the_case_is_not_trivial():
    """(a template with budget 0 has no match at a distance above 0: `every template` reads `every template with a
    budget` there; the one-cell template cannot have a budget, since a piece needs a literal cell of its own)"""
    tpls, ks, text, (kws, terms), rec, want = _main(1)
    _, _, text8, failing = _letters()
    w, d = want[0]["keyword_id"], want[1]
    print("symbols %d, keywords %d, records %d, matches %d, distances %s" % (text.size, len(kws), rec.size, w.size, np.bincount(d).tolist()))
    assert 3000 < text.size < 5000
    assert [len(t) for t in tpls[:len(LENGTHS)]] == list(LENGTHS) and sorted(set(ks)) == [0, 1, 3]
    for L, t in zip(LENGTHS, tpls):
        assert all(isinstance(t[i], SymbolClass) for i in (0, 15, 16, L - 1) if i < L and L > 1)
    for t in range(len(tpls)):
        assert np.any(d[w == t] == 0), t
        assert ks[t] == 0 or np.any(d[w == t] >= 1), t
        assert np.all(d[w == t] <= ks[t])
    # the copies: 0 to 4 failing cells, on class cells as well as on literals; within the budget they match at that distance
    got = {(int(r["end_pos"]), int(r["keyword_id"])): int(x) for r, x in zip(want[0], d)}
    on_class = on_literal = 0
    for t, at, cells in failing:
        assert got.get((at + len(tpls[t]) - 1, t)) == (len(cells) if len(cells) <= ks[t] else None), (t, at, cells)
        on_class += sum(not tc.is_literal(tpls[t][i]) for i in cells)
        on_literal += sum(tc.is_literal(tpls[t][i]) for i in cells)
    assert {len(cells) for t, at, cells in failing if ks[t] == 3} == {0, 1, 2, 3, 4} and on_class >= 8 and on_literal >= 8
    # a rejection that only a class cell causes: every literal cell accepts, and the class cells alone exceed the budget
    only_class = [(t, at) for t, at, cells in failing if len(cells) > ks[t] and all(not tc.is_literal(tpls[t][i]) for i in cells)]
    assert only_class and all((at + len(tpls[t]) - 1, t) not in got for t, at in only_class)
    S = want[0]["end_pos"].astype(np.int64) + 1 - want[0]["length"].astype(np.int64)
    n_seeds = np.array([tc.seeds_of(rec, terms, int(S[j]), int(w[j])) for j in range(w.size)])
    assert np.count_nonzero(n_seeds > 1) >= 2 and np.all(n_seeds >= 1)
    n = len(tpls)
    last = want[0][w >= n - 3]                                                   # (the one-cell template may end there too)
    ends, counts = np.unique(last["end_pos"], return_counts=True)
    tie = last[last["end_pos"] == ends[np.argmax(counts)]]
    assert [(int(r["length"]), int(r["keyword_id"])) for r in tie] == [(9, n - 1), (8, n - 3), (8, n - 2)]   # length descending, then template id


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_templates_on_every_symbol_size(torch_cuda, sb):
    tpls, ks, text, cut, rec, want = _main(sb)
    m, tset = _machine(sb, tpls, ks, cut)
    plan = m.plan(0)
    dev = _dev(torch_cuda, text)
    T = plan.templates_create(tset)
    info = T.info()
    assert info["templates"] == len(tpls) and info["terms"] == tset.terms.shape[0] == 2 + 7 * 4 + 3 * 2 and info["longest"] == 300
    assert info["max_k"] == 3 and info["seed_keywords"] == len(cut[0]) and info["classes"] == len(tset.classes) >= 10 and info["max_postings"] >= 1
    got, n, found = _scan(plan, dev, T, rec.size)
    assert found == rec.size and n == want[0].size
    same(got, want, sb)
    # the pass alone on tests/brute.py's records, with the compiled set and with a set compiled for the call
    same(_join(plan, rec, T, dev)[0], want, sb)
    same(_join(plan, rec, tset, dev)[0], want, sb)
    # nonzero pos_base
    shifted = rec.copy()
    shifted["end_pos"] += 5000
    same(_scan(plan, dev, T, rec.size, pos_base=5000)[0], _moved(want, 5000), sb)
    same(_join(plan, shifted, T, dev, pos_base=5000)[0], _moved(want, 5000), sb)
    # the text at an address that is no multiple of 16 (for bytes: an odd one)
    room = torch_cuda.zeros(text.size + 1, dtype=dev.dtype, device="cuda")
    room[1:] = dev
    assert room[1:].data_ptr() % 16 == sb and room[1:].is_contiguous()
    same(_join(plan, rec, T, room[1:])[0], want, sb)
    # host memory in, blocking; the machine's own call on the GPU path
    same(plan.scan_templates_host(text, tset), want, sb)
    same(plan.scan_templates_host(text, tset, pos_base=5000), _moved(want, 5000), sb)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_templates_host(text, tset, out_capacity=want[0].size - 1)
    assert e.value.code == E_OVERFLOW
    same(m.scan_templates(text, tset), want, sb)
    assert m.scan_path == PATH_GPU
    n_t = len(tpls)
    wrong = TemplateSet([tpls[n_t - 3]], [1], [[(0, 0, 2), (1, 2, 2)]], sym_size=sb)    # keywords 0 and 1 are pieces of other templates
    with pytest.raises(acm.ACMError) as e:
        m.scan_templates(text, wrong)
    assert e.value.code == E_ARG                                                  # the machine's call knows the spellings
    # an empty text, a text without a record
    assert plan.scan_templates_host(np.zeros(0, DTYPE[sb]), tset)[0].size == 0
    got, n, found = _scan(plan, _dev(torch_cuda, np.full(3000, HIGH[sb] | ord("q"), DTYPE[sb])), T, 16)
    assert (n, found) == (0, 0)
    T.close()
    plan.status()


@pytest.mark.parametrize("sb", [1, 2, 4, 8])
def test_class_edges_on_every_symbol_size(torch_cuda, sb):
    """one template k X m (and k X X m with budget 1) per class X; the text holds k x m and k x x m for every symbol x
    of interest: for bytes the classes that hold exactly 0x00, 0x1F, 0x20 (a word seam of the bitmap), both, 0xFF; for
    wider symbols range ends at 0 and at the type's maximum, and a range that lies wholly in the high bytes; the empty
    class, and the negated empty class, which accepts everything"""
    hi, top = HIGH[sb], (1 << (8 * sb)) - 1
    k_, m_ = hi | ord("k"), hi | ord("m")
    if sb == 1:
        sets = [[0], [0x1F], [0x20], [0x1F, 0x20], [0xFF], [(0x20, 0x3F)], [(0xE0, 0xFF)], [0, 0xFF], [(0x1F, 0x20)], [(0, 31), (64, 95), (128, 159), (224, 255)]]
        values = [0, 1, 0x1E, 0x1F, 0x20, 0x21, 0x3F, 0x40, 0x5F, 0x60, 0x7F, 0x80, 0x9F, 0xDF, 0xE0, 0xFE, 0xFF]
    else:
        sets = [[0], [top], [0, top], [(hi | 0x30, hi | 0x39)], [(0, hi)], [(hi | 0x100 if sb > 2 else hi | 0x80, top)], [(1, top - 1)],
                [(0x30, 0x39), (top - 9, top)]]
        values = [0, 1, 0x35, hi, hi | 0x35, hi | 0x2F, hi | 0x30, hi | 0x39, hi | 0x3A, hi | 0x80, (hi | 0x100) & top, top - 10, top - 9, top - 1, top]
    classes = [SymbolClass(s, neg) for s in sets for neg in (False, True)] + [SymbolClass([(0, top)], negate=True), SymbolClass([]), SymbolClass([], negate=True)]
    tpls = [[k_, c, m_] for c in classes] + [[k_, c, classes[(i + 3) % len(classes)], m_] for i, c in enumerate(classes)]
    ks = [0] * len(classes) + [1] * len(classes)
    text = np.array([s for x in values for s in (k_, x, m_)] + [s for x in values for y in (values[0], values[-1], x) for s in (k_, x, y, m_, k_)], DTYPE[sb])
    kws, terms = tc.compile_templates(tpls, ks)
    rec = tc.brute(kws, text)
    want = tc.templates(rec, text, tpls, ks, terms)
    same(want, tc.window_scan(text, tpls, ks), "the two derivations")
    per = np.bincount(want[0]["keyword_id"], minlength=len(tpls))
    print("sb %d: classes %d, symbols %d, records %d, matches %d, distances %s" % (sb, len(classes), text.size, rec.size, want[0].size, np.bincount(want[1]).tolist()))
    assert per[len(classes) - 3:len(classes)].tolist() == [0, 0, len(values)]     # everything negated and the empty class accept nothing, the negated empty class everything
    assert np.count_nonzero(per[:len(classes) - 3]) == len(classes) - 3 and np.count_nonzero(want[1]) > len(values)
    m = acm.Machine(sb)
    tset = TemplateSet.from_templates(m, tpls, ks)
    assert len(tset.classes) == len(classes) and [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws
    plan = m.plan(0)
    got, n, found = _scan(plan, _dev(torch_cuda, text), tset, rec.size)
    assert found == rec.size
    same(got, want, sb)
    same(plan.scan_templates_host(text, tset), want, sb)
    plan.status()


def _planted(m, o, body, sb, rng):
    """templates cut from `body` with class cells in them, copies with 0 to k + 1 failing cells in front of the body; the
    oracle gets the machine's new pieces under the same ids.  Returns (templates, budgets, the buffer, the set, its terms)."""
    dt = DTYPE[sb]
    stranger, top = (250 if sb == 1 else 0xFFFFF0), (1 << (8 * sb)) - 1           # (the stranger is in no template)

    def cells_of(sym, at):
        cells = [int(x) for x in sym]
        for j, i in enumerate(at):
            v = cells[i]
            cells[i] = [SymbolClass([(v, v), (stranger + 1, stranger + 2)]), SymbolClass([(stranger, stranger)], negate=True), ANY,
                        SymbolClass([(max(v, 1) - 1, min(v + 1, top))])][j % 4]
        return cells
    tpls = [cells_of(body[100:120], (0, 7, 15, 19)), cells_of(body[1000:1033], (3, 16, 17, 32)), cells_of(body[2000:2007], (2,))]
    ks = [2, 3, 1]
    planted = []
    for t, sym, k in zip(tpls, (body[100:120], body[1000:1033], body[2000:2007]), ks):
        can_fail = [i for i, c in enumerate(t) if c is not ANY]
        for d in range(k + 2):
            copy = sym.copy()
            copy[rng.choice(can_fail, size=d, replace=False)] = dt(stranger)
            planted += [copy, body[3000:3011]]
    buf = np.concatenate(planted + [body]).astype(dt)
    before = m.nb_keywords
    tset = TemplateSet.from_templates(m, tpls, ks)
    for i in range(before, m.nb_keywords):
        o.add_keyword(np.array(m.keyword(i)[0], dt))
    assert o.nb_keywords == m.nb_keywords
    terms = [[tuple(int(x) for x in tset.terms[i]) for i in range(int(tset.tgt_ptr[w]), int(tset.tgt_ptr[w + 1]))] for w in range(len(tpls))]
    return tpls, ks, buf, tset, terms


@pytest.mark.parametrize("name", ["dense", "gram", "starts"])
def test_scan_templates_on_plan_kinds(torch_cuda, monkeypatch, kat, name):
    m, o, text, make_plan, plan_ok, _ = kind(name, monkeypatch, kat)
    sb = m.sym_size
    tpls, ks, buf, tset, terms = _planted(m, o, text[:4096].astype(DTYPE[sb]), sb, np.random.default_rng(75))
    plan = make_plan(0)
    assert plan_ok(plan), plan.describe()                                        # (the family, through ACMPlanInfo)
    rec = o.scan(buf)
    want = tc.templates(rec, buf, tpls, ks, terms)
    same(want, tc.window_scan(buf, tpls, ks), "the two derivations")
    print("%s: records %d, matches %d, distances %s" % (name, rec.size, want[0].size, np.bincount(want[1]).tolist()))
    assert want[0].size >= 3 + 4 + 2 + 3 and np.count_nonzero(want[1]) >= 6
    got, n, found = _scan(plan, _dev(torch_cuda, buf), tset, rec.size)
    assert found == rec.size
    same(got, want, name)
    plan.status()


def test_plans_that_intern_8_byte_symbols_are_taken_and_class_plans_refused(torch_cuda, monkeypatch, kat):
    m, o, text, make_plan, plan_ok, _ = kind("u64", monkeypatch, kat)
    body = text[:3000]
    sym = body[500:517].copy()
    cells = [int(x) for x in sym]
    cells[4] = SymbolClass([(cells[4], cells[4]), (1 << 60, (1 << 61) - 1)])      # the second range lies outside the dictionary's symbols
    cells[9] = SymbolClass([(0, (1 << 64) - 1)])
    tpls, ks = [cells], [2]
    buf = body.copy()
    buf[1000:1017] = sym
    buf[1004] = np.uint64((1 << 60) + 5)                                          # interned to `unknown` by the scan; the class takes it by value
    buf[1500:1517] = sym
    buf[[1501, 1504, 1516]] = np.uint64(12345)
    buf[2000:2017] = sym
    buf[[2001, 2016]] = np.uint64(12345)
    before = m.nb_keywords
    tset = TemplateSet.from_templates(m, tpls, ks)
    for i in range(before, m.nb_keywords):
        o.add_keyword(np.array(m.keyword(i)[0], np.uint64))
    terms = [[tuple(int(x) for x in t) for t in tset.terms]]
    plan = make_plan(0)
    rec = o.scan(buf)
    want = tc.templates(rec, buf, tpls, ks, terms)
    same(want, tc.window_scan(buf, tpls, ks), "the two derivations")
    assert want[1].tolist() == [0, 0, 2]
    got, n, found = _scan(plan, _dev(torch_cuda, buf), tset, rec.size)
    assert found == rec.size
    same(got, want)
    plan.status()
    mc, _, _, make_classes, _, _ = kind("classes", monkeypatch, kat)
    classes = make_classes(0)
    with pytest.raises(acm.ACMError) as e:
        classes.templates_create(TemplateSet([binding.template("dallo[uw]ay")], [0], [[(5, 0, 5)]]))
    assert e.value.code == E_INELIGIBLE                                           # verification is by value on the caller's text
    # a set made for another plan's symbols: the calls that would be refused need no scratch; a target set is no template set
    T, L = plan.templates_create(tset), acm.lib()
    assert L.acm_gpu_templates_tmp_bytes(plan.h, T.h, 64, 64, 0) > 0 and L.acm_gpu_scan_templates_tmp_bytes(plan.h, T.h, 64, 64, 64, 0) > 0
    assert L.acm_gpu_templates_tmp_bytes(classes.h, T.h, 64, 64, 0) == 0 and L.acm_gpu_scan_templates_tmp_bytes(classes.h, T.h, 64, 64, 64, 0) == 0
    assert L.acm_gpu_templates_tmp_bytes(plan.h, None, 64, 64, 0) == 0
    one = torch_cuda.zeros(64, dtype=torch_cuda.int64, device="cuda")
    assert L.acm_gpu_scan_templates_device(classes.h, T.h, one.data_ptr(), 8, 0, None, 0, 4, one.data_ptr(), None, 1, one.data_ptr(), one.data_ptr() + 8,
                                           one.data_ptr(), 512, None) == E_ARG
    T.close()


def test_text_boundaries_of_a_packed_batch(torch_cuda):
    tpls, ks, text, cut, rec, want = _main(1)
    kws, terms = cut
    _, _, _, failing = _letters()
    exact = {w: at for w, at, cells in failing if not cells}
    inside = exact[4] + 11                                                       # a cut inside the exact copy of template 4
    at_begin, at_end = exact[5], exact[5] + 32                                   # a text that is the exact copy of template 5, begin to end
    off = np.array(sorted([0, 0, 9, inside, at_begin, at_end, at_end, 3000, text.size, text.size]), np.uint64)
    cut_want = tc.templates(rec, text, tpls, ks, terms, off)
    same(cut_want, tc.window_scan(text, tpls, ks, off), "the two derivations")
    whole = {tuple(int(x) for x in r) for r in want[0]}
    kept = {tuple(int(x) for x in r) for r in cut_want[0]}
    assert (inside - 11 + 30, 31, 4) in whole - kept and (at_end - 1, 32, 5) in kept and 0 < len(kept) < len(whole)
    # the seeds at the buffer's two ends: a piece of template 1 whose template would begin in front of the buffer, a piece of template 2
    # whose template would end behind it
    starts = {int(r["end_pos"]) + 1 - int(r["length"]) - o for r in rec for w in (1, 2) for kid, o, n in terms[w] if (kid, n) == (int(r["keyword_id"]), int(r["length"]))}
    assert min(starts) < 0 and max(starts) + len(tpls[2]) > text.size
    m, tset = _machine(1, tpls, ks, cut)
    plan = m.plan(0)
    dev, d_off = _dev(torch_cuda, text), _dev(torch_cuda, off.astype(np.int64))
    same(_join(plan, rec, tset, dev, offsets=d_off)[0], cut_want)
    same(_join(plan, rec, tset, dev)[0], want)
    got, n, found = _scan(plan, dev, tset, rec.size, offsets=d_off)
    assert found == rec.size
    same(got, cut_want)
    same(plan.scan_templates_host(text, tset, offsets=off), cut_want)
    same(m.scan_templates(text, tset, offsets=off), cut_want)
    with pytest.raises(acm.ACMError) as e:
        plan.scan_templates_host(text, tset, offsets=[0, 9, 5, text.size])
    assert e.value.code == E_ARG
    plan.status()                                                                 # a seed that points outside its text is no error


def test_more_records_than_the_grid_has_groups(torch_cuda, monkeypatch):
    """tiles of 64 records and more tiles than a capped grid has blocks (8 per CU): blocks stride over tiles"""
    monkeypatch.setenv("ACM_GPU_TEMPLATES_TILE", "64")
    ab, nb = SymbolClass([(97, 98)]), SymbolClass([98], negate=True)
    tpls, ks = [[97, 98, ab, 97, 98], [98, nb, 98, 97, ANY], [97, 97, SymbolClass([98])]], [1, 1, 0]
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    n = ((8 * cus + 3) * 64 + 65) * 2
    text = bytes(np.random.default_rng(8).choice(np.frombuffer(b"ab", np.uint8), size=n))
    m = acm.Machine(1)
    tset = TemplateSet.from_templates(m, tpls, ks)
    kws, terms = tc.compile_templates(tpls, ks)
    rec = tc.oracle_records([bytes(kw) for kw in kws], text)
    assert rec.size > (8 * cus + 2) * 64 + 65
    want = tc.window_scan(text, tpls, ks)
    head = rec[rec["end_pos"] < 3000]
    part = tc.templates(head, text[:3000], tpls, ks, terms)
    same(part, tc.window_scan(text[:3000], tpls, ks), "the two derivations, where the loop is affordable")
    plan = m.plan(0)
    got, cnt = _join(plan, rec, tset, _dev(torch_cuda, text), out_capacity=want[0].size)
    same(got, want)
    assert n // 8 < want[0].size
    plan.status()


def test_out_capacity_counts_on_the_device_and_overflow(torch_cuda):
    torch = torch_cuda
    tpls, ks, text, cut, rec, want = _main(1)
    m, tset = _machine(1, tpls, ks, cut)
    plan = m.plan(0)
    T = plan.templates_create(tset)
    dev = _dev(torch, text)
    total = want[0].size
    assert total > 30
    sentinel = np.zeros(total + 8, po.RECORD_DTYPE)
    sentinel["end_pos"], sentinel["length"], sentinel["keyword_id"] = SENTINEL, 7, 7

    def join(out_capacity, count=None, room=None):
        d_out = _rec_dev(torch, sentinel)
        d_dist = torch.full((total + 8,), 0x5A5A, dtype=torch.int32, device="cuda")
        d_rec = _rec_dev(torch, rec, room, fill=SENTINEL)
        out, dist, cnt = plan.templates_records(d_rec, rec.size if room is None else room, T, dev, out=d_out, dist=d_dist, out_capacity=out_capacity, count=count)
        return _rec_host(d_out, sentinel.size), _dist_host(d_dist, total + 8), int(cnt.item())
    # the exact room; one short: the count is the need and nothing is written; no room: the count alone
    out, dist, n = join(total)
    assert n == total and np.array_equal(out[total:], sentinel[total:]) and np.all(dist[total:] == 0x5A5A)
    same((out[:n], dist[:n]), want)
    out, dist, n = join(total - 1)
    assert n == total and np.array_equal(out, sentinel) and np.all(dist == 0x5A5A)
    out, dist, n = join(0)
    assert n == total and np.array_equal(out, sentinel) and np.all(dist == 0x5A5A)
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
    got, n, found = _scan(plan, dev, T, rec.size - 1, out_capacity=total)
    assert n == 0 and found == rec.size
    got, n, found = _scan(plan, dev, T, found, out_capacity=total)
    assert found == rec.size
    same(got, want)
    got, n, found = _scan(plan, dev, T, 0, out_capacity=total)                    # no room at all: the scan's count
    assert n == 0 and found == rec.size
    got, n, found = _scan(plan, dev, T, rec.size, out_capacity=total - 1)         # the records fit, the matches do not
    assert n == total and found == rec.size
    # dist may be NULL
    L = acm.lib()
    d_rec, d_out, cnt = _rec_dev(torch, rec), _rec_dev(torch, sentinel), torch.zeros(1, dtype=torch.int64, device="cuda")
    tb = L.acm_gpu_templates_tmp_bytes(plan.h, T.h, rec.size, total, 0)
    tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    assert L.acm_gpu_templates_records_device(plan.h, T.h, d_rec.data_ptr(), rec.size, None, dev.data_ptr(), text.size, 0, None, 0, d_out.data_ptr(), None,
                                              total, cnt.data_ptr(), tmp.data_ptr(), tb, None) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == total and np.array_equal(_rec_host(d_out, total), want[0])
    # refused calls, and what they would need
    assert tb > 0 and L.acm_gpu_templates_tmp_bytes(plan.h, T.h, 1 << 31, 0, 0) == 0 and L.acm_gpu_templates_tmp_bytes(plan.h, T.h, 64, 1 << 31, 0) == 0

    def call(templates_h=T.h, records=d_rec.data_ptr(), n=rec.size, text_ptr=dev.data_ptr(), out=d_out.data_ptr(), cap=total, count=cnt.data_ptr(),
             scratch=tmp.data_ptr(), tmp_bytes=tb):
        return L.acm_gpu_templates_records_device(plan.h, templates_h, records, n, None, text_ptr, text.size, 0, None, 0, out, None, cap, count, scratch, tmp_bytes, None)
    assert call(templates_h=None) == E_ARG and call(records=None) == E_ARG and call(text_ptr=None) == E_ARG and call(out=None) == E_ARG
    assert call(count=None) == E_ARG and call(scratch=None) == E_ARG and call(tmp_bytes=tb - 1) == E_ARG and call(n=1 << 31) == E_ARG
    assert call(cap=1 << 31) == E_ARG and call(out=d_rec.data_ptr()) == E_ARG     # d_out overlapping d_records
    T.close()
    plan.status()


def test_offsets_that_break_the_contract_match_nothing(torch_cuda):
    torch = torch_cuda
    tpls, ks, text, cut, rec, want = _main(1)
    m, tset = _machine(1, tpls, ks, cut)
    n = text.size
    sentinel = np.zeros(want[0].size, po.RECORD_DTYPE)
    sentinel["end_pos"] = SENTINEL
    dev = _dev(torch, text)
    for what, off in (("decreasing", [0, 40, 30, n]), ("first not 0", [1, 40, n]), ("last not n", [0, 40, n - 1]), ("far out", [0, 1 << 60, n])):
        plan = m.plan(0)
        plan.status()
        d_out = _rec_dev(torch, sentinel)
        out, dist, cnt = plan.templates_records(_rec_dev(torch, rec), rec.size, tset, dev, offsets=_dev(torch, np.array(off, np.int64)), out=d_out)
        assert int(cnt.item()) == 0, what
        assert np.array_equal(_rec_host(d_out, sentinel.size), sentinel), what
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_records_that_break_the_contract_are_skipped_and_reported(torch_cuda):
    tpls, ks, text, cut, rec, want = _main(1)
    m, tset = _machine(1, tpls, ks, cut)
    pos_base = 1000
    shifted = rec.copy()
    shifted["end_pos"] += pos_base
    dev = _dev(torch_cuda, text)
    kid = 0                                                                       # (a keyword that seeds templates: the record would be looked at)
    bad = {"a start below pos_base": (pos_base + 1, 4, kid), "a length of 0": (pos_base + 20, 0, kid), "beyond the buffer": (pos_base + text.size, 1, kid),
           "below pos_base": (pos_base - 1, 1, kid), "far beyond": (1 << 62, 3, kid)}
    for what, triple in bad.items():
        plan = m.plan(0)
        plan.status()
        mixed = np.concatenate([shifted, np.array([triple], po.RECORD_DTYPE)])
        mixed = mixed[np.lexsort((-mixed["length"].astype(np.int64), mixed["end_pos"]))]   # canonical order with the stranger in it
        same(_join(plan, mixed, tset, dev, pos_base=pos_base)[0], _moved(want, pos_base), what)
        with pytest.raises(acm.ACMError) as e:
            plan.status()
        assert e.value.code == E_INTERNAL, what
        plan.close()


def test_a_pending_delta_after_plan_update(torch_cuda):
    tpls, ks, text, cut, rec, want = _main(1)
    n_t = len(tpls)
    m = acm.Machine(1)
    early = TemplateSet.from_templates(m, tpls[n_t - 3:n_t - 2], ks[n_t - 3:n_t - 2])
    plan = m.plan(0)
    T0 = plan.templates_create(early)
    tset = TemplateSet.from_templates(m, tpls, ks)                                # more pieces: the machine is ahead of the plan
    with pytest.raises(acm.ACMError) as e:
        plan.templates_create(tset)
    assert e.value.code == E_ARG                                                  # the plan does not know them yet
    plan.update(m)
    T = plan.templates_create(tset)
    words = [m.keyword(i)[0] for i in range(m.nb_keywords)]
    terms = [[tuple(int(x) for x in tset.terms[i]) for i in range(int(tset.tgt_ptr[w]), int(tset.tgt_ptr[w + 1]))] for w in range(n_t)]
    assert terms != cut[1]                                                        # (other ids than the plain cut's: the records are made anew)
    rec2 = tc.brute(words, text)
    same(tc.templates(rec2, text, tpls, ks, terms), want, "the same matches under other keyword ids")
    dev = _dev(torch_cuda, text)
    got, n, found = _scan(plan, dev, T, rec2.size)
    assert found == rec2.size
    same(got, want)
    # the set made before the update stays valid
    same(_scan(plan, dev, T0, rec2.size)[0], tc.window_scan(text, tpls[n_t - 3:n_t - 2], ks[n_t - 3:n_t - 2]))
    same(m.scan_templates(text, tset), want)
    T.close()
    T0.close()
    plan.status()


def test_three_templates_of_the_novel(torch_cuda, novel_bytes):
    text = novel_bytes[:8192] + b" 078-05-1120, 219-09-9999; " + bytes([0x45, 0x3A, 0, 0xC3, 0x41, 0x45, 0x30, 0xFF, 0x13, 0x4F, 0x45, 0x40, 0, 0x13, 0x41])
    tpls = [binding.template(r"[A-Z][a-z]{2}\.\sDalloway"), binding.template(r"\d{3}-\d{2}-\d{4}"), binding.template(r"th[aeiou]\s\w"),
            binding.hex_template("45 3? ?? ?3 [41-4F]")]
    ks = [1, 0, 0, 0]
    m = acm.Machine(1)
    tset = TemplateSet.from_templates(m, tpls, ks)
    kws, terms = tc.compile_templates(tpls, ks)
    assert [m.keyword(i)[0] for i in range(m.nb_keywords)] == kws
    want = tc.window_scan(text, tpls, ks)
    assert np.array_equal(tc.regex_scan(rb"\d{3}-\d{2}-\d{4}", text, 11)[0]["end_pos"], want[0]["end_pos"][want[0]["keyword_id"] == 1])
    per = np.bincount(want[0]["keyword_id"], minlength=len(tpls))
    print("matches per template %s, distances %s" % (per.tolist(), np.bincount(want[1]).tolist()))
    assert np.all(per[:3] >= 2) and per[3] == 2
    plan = m.plan(0)
    rec = tc.oracle_records([bytes(kw) for kw in kws], text)
    got, n, found = _scan(plan, _dev(torch_cuda, text), tset, rec.size)
    assert found == rec.size
    same(got, want)
    same(m.scan_templates(text, tset), want)
    plan.status()
