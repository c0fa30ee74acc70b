"""Dense kernel, continuation mode: the slow side of a step.  hotfail of the rowless states lies in
LDS in descending order below a fixed address, both streams of a lane read theirs in the same step,
one queue bookkeeping serves both streams, and the last run-over step is skipped when no lane of
the wave is still inside a match before it.  Every case compares the full record set (sorted on
the host) and the count-only total with the CPU oracle; the oracle's own answer is checked against
the plantings first (that part needs no GPU)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests.cases import build_pair

CHUNK = 64                 # bytes per lane-stream chunk
STRIDE = 64 * CHUNK        # distance between the chunks of a lane's two streams
TILE = 2 * STRIDE          # bytes per wave tile
N = (1 << 20) + 37         # ragged; 128 tiles and a bit: several blocks and the tile pool
RUNOVER = 4                # straight-line steps past a chunk
AZ = np.arange(97, 123, dtype=np.uint8)
EIGHT = b"qzjxvkwy"        # 8 letters: repeated, all 64 lanes of a wave are in phase


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    torch.cuda.set_device(0)
    return torch


def _dictionary():
    """about 600 a-z keywords of 6-12 letters (more states than LDS rows) and EIGHT"""
    rng = np.random.default_rng(601)
    kws = sorted({bytes(rng.choice(AZ, size=int(rng.integers(6, 13)))) for _ in range(600)})
    return kws + [EIGHT]


_pair = None


def _big_pair():
    global _pair
    if _pair is None:
        kws = _dictionary()
        m, o = build_pair(kws, 1)
        _pair = (kws, m, o)
    return _pair


def _spell(flat, state):
    """the symbols on the trie path from the root to `state`, and a keyword that path leads into"""
    n = flat.info.n_states
    parent = np.zeros(n, np.int64)
    sym = np.zeros(n, np.uint8)
    for s in range(n):
        for e in range(int(flat.row_ptr[s]), int(flat.row_ptr[s + 1])):
            parent[flat.edge_next[e]] = s
            sym[flat.edge_next[e]] = flat.edge_sym[e]
    path, s = [], state
    while s:
        path.append(int(sym[s]))
        s = int(parent[s])
    path = bytes(reversed(path))
    s, full = state, bytearray(path)
    while flat.term_kw[s] == 0xFFFFFFFF:  # down the first edge until a keyword ends
        e = int(flat.row_ptr[s])
        full.append(int(flat.edge_sym[e]))
        s = int(flat.edge_next[e])
    return path, bytes(full)


class Planter:
    def __init__(self, n, seed):
        self.text = np.random.default_rng(seed).choice(AZ, size=n)
        self.ends = []   # (end position, keyword) of every whole keyword planted

    def put(self, start, word, whole=True):
        w = np.frombuffer(word, np.uint8)
        assert start >= 0 and start + w.size <= self.text.size
        self.text[start:start + w.size] = w
        if whole:
            self.ends.append((start + w.size - 1, word))


def _rowless_text(flat, hd):
    """the keywords through the first rowless state (hd) and the last state, and the bare paths to
    them, at every offset of a chunk and with 1 .. 5 symbols past a chunk end"""
    n = flat.info.n_states
    p = Planter(N, 602)
    cur = CHUNK   # a chunk boundary; everything before it is settled
    for state in (hd, n - 1):
        path, full = _spell(flat, state)
        assert len(path) == flat.depth[state] and full.startswith(path)
        for word, whole in ((full, True), (path, path == full)):
            for off in range(CHUNK):             # every offset 0 .. 63 of a chunk
                p.put(cur + off, word, whole)
                cur += 3 * CHUNK
            for past in range(1, RUNOVER + 2):   # live at the last run-over step, dead before it, a walk item
                for boundary in (CHUNK, STRIDE, TILE):
                    end = (cur + CHUNK) // boundary * boundary + boundary
                    p.put(end - len(word) + past, word, whole)
                    cur = end + 2 * CHUNK
    assert cur < N
    return p


def _two_streams_text(flat, hd):
    """the same keyword at p and at p + the stream stride: both streams of a lane step into a rowless
    state in the same step"""
    p = Planter(N, 603)
    _, full = _spell(flat, flat.info.n_states - 1)
    _, first = _spell(flat, hd)
    i = 0
    for tile in range(0, N // TILE - 1):
        for word in (full, first):
            at = tile * TILE + (7 * i % 61) * CHUNK + (5 * i % CHUNK)
            if at + STRIDE + len(word) < N and at % STRIDE + len(word) + CHUNK < STRIDE:
                p.put(at, word)
                p.put(at + STRIDE, word)
            i += 1
    return p


def _repeated_text():
    """EIGHT over and over: every eighth step all 128 lane-streams of a wave have an item"""
    p = Planter(N, 604)
    reps = N // len(EIGHT)
    p.text[:reps * len(EIGHT)] = np.frombuffer(EIGHT * reps, np.uint8)
    p.ends = [(i * len(EIGHT) + len(EIGHT) - 1, EIGHT) for i in range(reps)]
    return p


def _emit_window_case():
    """the dictionary with B = A[1:] + 'k' added (A: the keyword of the last state): A ends at
    emit_from - 1 (not reported), B at emit_from; the last keyword ends at the text's last byte"""
    kws, m, _ = _big_pair()
    flat = m.flatten()
    _, a = _spell(flat, flat.info.n_states - 1)
    b = a[1:] + b"k"
    emit_from = 5 * TILE + 3 * CHUNK + 1
    p = Planter(N, 605)
    p.put(emit_from - len(a), a + b"k", whole=False)
    p.put(N - len(a), a)
    for i in range(40):   # and the same pair around chunk ends further on, inside the window
        p.put(emit_from + (20 * i + 7) * CHUNK - 3, a + b"k", whole=False)
    return kws + [b], p, emit_from, a, b


def _sorted(records):
    return np.sort(np.ascontiguousarray(records, dtype=po.RECORD_DTYPE), order=["end_pos", "length", "keyword_id"])


def _oracle_records(o, p, emit_from=0):
    """the oracle's records; every planted keyword is among them"""
    want = _sorted(o.scan(p.text, emit_from=emit_from))
    have = set(zip(want["end_pos"].tolist(), want["length"].tolist()))
    for end, word in p.ends:
        assert (end >= emit_from) == ((end, len(word)) in have), (end, word)
    return want


def _check_gpu(torch, plan, p, want, emit_from=0):
    dev = torch.from_numpy(np.ascontiguousarray(p.text)).cuda()
    rec, cnt = plan.scan(dev, emit_from=emit_from, capacity=want.size + 64)
    n = int(cnt.item())
    assert n == want.size
    got = _sorted(np.frombuffer(rec[:n].cpu().numpy().tobytes(), dtype=po.RECORD_DTYPE))
    assert np.array_equal(got, want)
    assert int(plan.count(dev, emit_from=emit_from).item()) == want.size
    plan.status()


def _short_case(lmax):
    rng = np.random.default_rng(610 + lmax)
    ab = np.arange(97, 101, dtype=np.uint8)
    kws = {bytes(rng.choice(ab, size=int(rng.integers(2, lmax + 1)))) for _ in range(5)}
    kws |= {b"a" * lmax, (b"ab" * lmax)[:lmax]}
    p = Planter(N, 620 + lmax)
    p.text = rng.choice(ab, size=N)
    for i, b in enumerate(range(CHUNK, N - CHUNK, 5 * CHUNK)):   # a keyword of lmax symbols across chunk ends
        p.put(b - 1 - i % lmax, b"a" * lmax)
    p.text[N - lmax:] = 97
    p.ends.append((N - 1, b"a" * lmax))
    return sorted(kws), p


# ---- the oracle alone: what the cases expect is what they plant (no GPU)

def test_oracle_finds_what_the_cases_plant():
    kws, m, o = _big_pair()
    flat = m.flatten()
    n = flat.info.n_states
    assert n > 3000 and int(flat.depth[n - 1]) == 12
    hd = n // 2   # any state in the middle stands in for the first rowless one here
    for p in (_rowless_text(flat, hd), _two_streams_text(flat, hd), _repeated_text()):
        assert len(p.ends) > 100
        assert _oracle_records(o, p).size >= len(p.ends)
    assert _oracle_records(o, _repeated_text()).size == N // len(EIGHT)
    ekws, p, emit_from, a, b = _emit_window_case()
    _, o2 = build_pair(ekws, 1)
    want = _oracle_records(o2, p, emit_from)
    ends = set(zip(want["end_pos"].tolist(), want["length"].tolist()))
    assert (emit_from - 1, len(a)) not in ends and (emit_from, len(b)) in ends and (N - 1, len(a)) in ends
    assert int(want["end_pos"].min()) >= emit_from and int(want["end_pos"].max()) == N - 1
    for lmax in (2, 3, 4, 5):
        skws, p = _short_case(lmax)
        assert max(len(k) for k in skws) == lmax
        _, o3 = build_pair(skws, 1)
        assert _oracle_records(o3, p).size > len(p.ends)


# ---- the kernel against the oracle

@pytest.fixture(scope="module")
def big_plan(torch_cuda):
    kws, m, o = _big_pair()
    plan = m.plan(0)
    d = plan.describe()
    assert d["kernel"] == 1 and d["entry_bytes"] == 2, d
    assert d["lds_hotfail"] > 0 and d["lds_rows"] + d["lds_hotfail"] == d["dense_rows"], d
    return m.flatten(), plan, o


@pytest.mark.gpu
def test_rowless_states_at_both_ends_of_the_hotfail_array(torch_cuda, big_plan):
    flat, plan, o = big_plan
    p = _rowless_text(flat, plan.info.lds_rows)
    _check_gpu(torch_cuda, plan, p, _oracle_records(o, p))


@pytest.mark.gpu
def test_both_streams_rowless_in_one_step(torch_cuda, big_plan):
    flat, plan, o = big_plan
    p = _two_streams_text(flat, plan.info.lds_rows)
    assert len(p.ends) > 200
    _check_gpu(torch_cuda, plan, p, _oracle_records(o, p))


@pytest.mark.gpu
def test_queue_passes_64_items_in_a_single_step(torch_cuda, big_plan):
    flat, plan, o = big_plan
    p = _repeated_text()
    _check_gpu(torch_cuda, plan, p, _oracle_records(o, p))


@pytest.mark.gpu
@pytest.mark.parametrize("lmax", [2, 3, 4, 5])
def test_fewer_runover_steps_than_the_kernel_has(torch_cuda, lmax):
    skws, p = _short_case(lmax)
    m, o = build_pair(skws, 1)
    plan = m.plan(0)
    assert plan.info.kernel == 1 and plan.info.entry_bytes == 2, plan.describe()
    _check_gpu(torch_cuda, plan, p, _oracle_records(o, p))


@pytest.mark.gpu
def test_emit_window_and_the_last_byte(torch_cuda):
    ekws, p, emit_from, a, b = _emit_window_case()
    m, o = build_pair(ekws, 1)
    plan = m.plan(0)
    assert plan.info.kernel == 1 and plan.info.lds_hotfail > 0, plan.describe()
    want = _oracle_records(o, p, emit_from)
    _check_gpu(torch_cuda, plan, p, want, emit_from)
