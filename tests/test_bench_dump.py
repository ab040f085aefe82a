"""bench.py --dump-outputs: the sampled read-back of the caller's buffers
(bench.dump_table) on the CPU against a table laid out by hand, and the files of
a plain `bench.py --config c1` run on the GPU against the library's own download
of the same table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _sb64(A, spans, value):
    """Buffers as build_blocks_into leaves them: span (b0, b1, s0) at slot s0, element
    (s, t) at ((s / 64 - b0) A + t) 64 + s % 64 of the span; value(s, t) per field."""
    nslot = sum(b1 - b0 for b0, b1, _ in spans)
    buf = np.full(nslot * A * 64, -7.0)
    for b0, b1, s0 in spans:
        for s in range(b0 * 64, min(A, b1 * 64)):
            for t in range(A):
                buf[s0 * A * 64 + ((s // 64 - b0) * A + t) * 64 + s % 64] = value(s, t)
    return buf


@pytest.mark.parametrize("A, sample", [(150, 1 << 20), (150, 4096)], ids=["whole", "sampled"])
def test_dump_table_reads_sb64_entries(tmp_path, monkeypatch, A, sample):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    nblk = (A + 63) // 64   # 3 blocks: two packed out of order, the last kept by another rank
    att = np.random.default_rng(1).permutation(1000)[:A].astype(np.int32)
    rec = _sb64(A, [(0, nblk, 0)], lambda s, t: s * 1000.0 + t)
    lr = torch.from_numpy(np.stack([rec, -rec], axis=1).copy())
    spans = [(1, 2, 0), (0, 1, 1)]
    nx = torch.from_numpy(_sb64(A, spans, lambda s, t: s + 2 * t).astype(np.int32))
    hp = torch.from_numpy(_sb64(A, spans, lambda s, t: 65000 - (s + t) % 50).astype(np.uint16).view(np.int16))
    out = str(tmp_path / "o")
    bench.dump_table(out, att, lr, nx, hp, spans, True, torch.device("cpu"))
    got = {k: np.load(os.path.join(out, k + ".npy")) for k in ("pairs", "lat", "rel", "next", "hops")}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    n = A * A if A * A <= sample else sample
    assert got["pairs"].shape == (n, 2) and all(got[k].shape == (n,) for k in ("lat", "rel", "next", "hops"))
    slot_of = {int(v): i for i, v in enumerate(att)}
    s = np.array([slot_of[int(v)] for v in got["pairs"][:, 0]])
    t = np.array([slot_of[int(v)] for v in got["pairs"][:, 1]])
    if n == A * A:
        assert (s == np.repeat(np.arange(A), A)).all() and (t == np.tile(np.arange(A), A)).all()
    np.testing.assert_array_equal(got["lat"], s * 1000.0 + t)
    np.testing.assert_array_equal(got["rel"], -(s * 1000.0 + t))
    own = s < 128
    assert own.any() and (~own).any()
    np.testing.assert_array_equal(got["next"][own], (s + 2 * t)[own])
    np.testing.assert_array_equal(got["hops"][own], (65000 - (s + t) % 50)[own])
    assert np.isnan(got["next"][~own]).all() and np.isnan(got["hops"][~own]).all()
    # the same sample every run; records this rank never received are NaN too
    out2 = str(tmp_path / "o2")
    bench.dump_table(out2, att, lr, nx, hp, spans, False, torch.device("cpu"))
    np.testing.assert_array_equal(np.load(os.path.join(out2, "pairs.npy")), got["pairs"])
    lat2 = np.load(os.path.join(out2, "lat.npy"))
    np.testing.assert_array_equal(lat2[own], got["lat"][own])
    assert np.isnan(lat2[~own]).all()


def test_write_outputs_bounds_the_total(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path), {"a": np.zeros(5_000_000), "b": np.zeros(5_000_000)})


@pytest.mark.gpu
@pytest.mark.engine_fixed
def test_plain_run_dumps_the_table_it_timed(tmp_path):
    """A plain run (no --full) times exactly --steps tables, carries no CPU baseline
    or side configs, and its files hold the whole C1 table entry for entry."""
    from shadow_amd import spe
    sys.path.insert(0, ROOT)
    import bench
    out = str(tmp_path / "o")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "c1all", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", out], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.rstrip("\n").splitlines()[-1])
    assert line["steps"] == 2 and len(line["rank0_step_s"]) == 2 and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None and "side_configs" not in line
    top, att, _ = bench.workload("c1all")
    g = spe.Graph(top)
    order = g.order_sources(att)
    t = spe.PathTable(g, order, exact_sources=False)
    t.build()
    ref = t.download()
    t.close()
    A = len(order)
    got = {k: np.load(os.path.join(out, k + ".npy")) for k in ("pairs", "lat", "rel", "next", "hops")}
    np.testing.assert_array_equal(got["pairs"][:, 0], np.repeat(order, A))
    np.testing.assert_array_equal(got["pairs"][:, 1], np.tile(order, A))
    for k in ("lat", "rel", "next", "hops"):
        np.testing.assert_array_equal(got[k].reshape(A, A), ref[k], err_msg=k)
