"""bench.py --dump-outputs on the host: the packed result rows come back out as the arrays Batch.results() returns, float32, within the
size cap (a fixed, seeded sample above it).  CPU only; the GPU run of bench.py writes through the same function."""
import os

import numpy as np

import bench
from dsp_slam_amd import distributed as D


def _rows(n, seed=3):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((n, 4, 4)).astype(np.float32)
    code = rng.standard_normal((n, 64)).astype(np.float32)
    loss = rng.random(n).astype(np.float32)
    status = rng.integers(0, 3, n).astype(np.int32)
    return D.pack_results(t, code, loss, status), (t, code, loss, status)


def test_dump_outputs_writes_what_results_returns(tmp_path):
    packed, (t, code, loss, status) = _rows(64)
    bench.dump_outputs(str(tmp_path), packed, D)
    assert sorted(os.listdir(str(tmp_path))) == ["code.npy", "loss.npy", "status.npy", "t_cam_obj.npy"]
    for name, want in (("t_cam_obj", t), ("code", code), ("loss", loss), ("status", status)):
        got = np.load(str(tmp_path / (name + ".npy")), allow_pickle=False)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want.astype(np.float32)), name


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    packed, (t, code, _, _) = _rows(1000)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * (82 * 4 + 8))
    bench.dump_outputs(str(tmp_path / "a"), packed, D)
    bench.dump_outputs(str(tmp_path / "b"), packed, D)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) - 128 for f in os.listdir(str(tmp_path / "a")))      # minus the .npy headers
    assert total <= bench.DUMP_MAX_BYTES
    idx = np.load(str(tmp_path / "a" / "object_index.npy"))
    assert idx.dtype == np.float64 and len(idx) == 100 and np.all(np.diff(idx) > 0)
    for f in os.listdir(str(tmp_path / "a")):
        assert np.array_equal(np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))), f
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(str(tmp_path / "a" / "t_cam_obj.npy")), t[i]) and np.array_equal(np.load(str(tmp_path / "a" / "code.npy")), code[i])
