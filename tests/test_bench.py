"""bench.py's plain line and `--dump-outputs`: the dump holds what the timed scan computed (the
oracle's records of the same text), in an order that does not depend on the scan's own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aho_corasick_1975_amd as acm
import bench
from oracle import pyoracle as po
from tests.conftest import ROOT


def _canonical(pos, length, kid):
    rec = np.stack([pos, length, kid], axis=1).astype(np.float64)
    return rec[np.lexsort((rec[:, 2], -rec[:, 1], rec[:, 0]))]


def test_dump_outputs_order_free_and_sampled_by_seed(tmp_path, monkeypatch):
    import torch
    rng = np.random.default_rng(1)
    n = 5000
    pos, length, kid = rng.integers(0, 1 << 24, n), rng.integers(1, 12, n), rng.integers(0, 100000, n)
    buf = torch.zeros((n + 16, 2), dtype=torch.int64)
    buf[:n, 0] = torch.from_numpy(pos)
    buf[:n, 1] = torch.from_numpy(length | (kid << 32))
    shuffled = buf.clone()
    shuffled[:n] = buf[:n][torch.from_numpy(rng.permutation(n))]
    for name, b in (("a", buf), ("b", shuffled)):
        bench.dump_outputs(str(tmp_path / name), b, n, 1 << 24)
    whole = np.load(tmp_path / "a" / "records.npy")
    assert whole.dtype == np.float64 and np.array_equal(whole, _canonical(pos, length, kid))
    assert np.array_equal(whole, np.load(tmp_path / "b" / "records.npy"))
    assert np.load(tmp_path / "a" / "count.npy").tolist() == [n]
    # above the limit: the same sample whatever the scan's order, a subset of the records, within the limit
    monkeypatch.setattr(bench, "DUMP_MAX_RECORDS", 1000)
    for name, b in (("c", buf), ("d", shuffled)):
        bench.dump_outputs(str(tmp_path / name), b, n, 1 << 24)
    c, d = np.load(tmp_path / "c" / "records.npy"), np.load(tmp_path / "d" / "records.npy")
    assert np.array_equal(c, d) and 0 < len(c) <= 1000
    assert set(map(tuple, c.tolist())) <= set(map(tuple, whole.tolist()))
    assert np.load(tmp_path / "c" / "count.npy").tolist() == [n]


@pytest.mark.gpu
def test_plain_line_and_dumped_records_against_the_oracle(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--mib", "16", "--prewarm-ms", "0", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["metric"]
    assert not {"roofline", "e2e", "cpu_baseline", "other_configs"} & set(line)
    kd, ko = acm.synth.keywords(1000)
    o = po.Oracle(1)
    o.add_keywords_packed(kd, ko)
    want = o.scan(acm.synth.text(16 << 20, kd, ko))
    assert np.load(out / "count.npy").tolist() == [want.size] == [line["config"]["matches_per_gpu"]]
    got = np.load(out / "records.npy")
    assert np.array_equal(got, _canonical(want["end_pos"], want["length"], want["keyword_id"]))
