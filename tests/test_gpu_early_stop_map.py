"""GPU: tools/reoptimise_map.py --tol -- a saved map re-optimised with the per-object convergence rule (dsp_batch_convergence): sharded ==
unsharded bit for bit, iteration counts included, and the histogram the tool prints is that of dsp_batch_iterations_used."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from dsp_slam_amd import fixtures, synth, engine as E
from dsp_slam_amd.map_objects import read_map_objects, write_map_objects

pytestmark = pytest.mark.gpu
TOL = (1e-2, 1e-2)


@pytest.fixture
def mirror():
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    sys.path.insert(0, pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    yield
    sys.path.remove(pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]


def _config(tmp_path):
    cars = fixtures.materialize_decoder_dir("cars", str(tmp_path / "cars_64"))
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    cfg["DeepSDF_DIR"] = cars
    cfg.setdefault("data_type", "KITTI")
    p = str(tmp_path / "cfg.json")
    with open(p, "w") as f:
        json.dump(cfg, f)
    return p


def _run_tool(name, argv):
    import runpy
    old = sys.argv
    sys.argv = [name] + argv
    try:
        runpy.run_path(os.path.join(ROOT, "tools", name), run_name="__main__")
    finally:
        sys.argv = old


def _make_map(tmp_path, n_obj):
    map_dir = tmp_path / "map"
    (map_dir / "observations").mkdir(parents=True)
    objs = []
    for i in range(n_obj):
        o = synth.make_object(7100 + i, n_surface=160 + 10 * i, n_background=40)
        t_wc = np.eye(4)
        t_wc[:3, 3] = (3.0 * i, 0.0, -2.0 * i)
        objs.append(dict(id=2 * i + 1, pose=t_wc @ o["t_cam_obj_init"].astype(np.float64), code=np.zeros(64, np.float32)))
        if i != 1:                      # object 1 has no observation: it keeps what the map holds and has no iteration count
            np.savez(map_dir / "observations" / ("%d.npz" % (2 * i + 1)), pts=o["pts"], rays=o["rays"], depth=o["depth"], t_world_cam=t_wc)
    write_map_objects(str(map_dir / "MapObjects.txt"), objs)
    return map_dir


def test_reoptimise_map_with_tolerances(tmp_path, mirror, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import reoptimise_map as R
    from deep_sdf.workspace import config_decoder
    cfg_path = _config(tmp_path)
    cfg = json.load(open(cfg_path))
    map_dir = _make_map(tmp_path, 6)
    dec = config_decoder(cfg["DeepSDF_DIR"]).cuda(0)
    eng, prm = dec.engine, E.params_from_configs(cfg)
    # the saved map becomes a warm start for half of its objects: re-optimised once without the rule, three objects written back
    objs = read_map_objects(str(map_dir / "MapObjects.txt"))
    obs = R.load_observations(str(map_dir), objs)
    first, st0 = R.reoptimise([eng], prm, objs, obs, 64)
    assert st0["iterations_used"] is None and st0["n_good"] == 5
    write_map_objects(str(map_dir / "MapObjects.txt"), first[:3] + objs[3:])
    objs = read_map_objects(str(map_dir / "MapObjects.txt"))
    whole, st1 = R.reoptimise([eng], prm, objs, obs, 64, tol=TOL)
    shard, st3 = R.reoptimise([eng], prm, objs, obs, 64, shards=[(0, 2), (2, 2), (2, 5)], tol=TOL)
    dec.engine.close()
    assert np.array_equal(st1["packed"], st3["packed"]) and np.array_equal(st1["iterations_used"], st3["iterations_used"])
    for a, b in zip(whole, shard):
        assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["code"], b["code"])
    used = st1["iterations_used"]
    assert used.shape == (5,) and used.min() < prm.num_iterations and used.min() >= 1, used
    assert np.array_equal(whole[1]["pose"], objs[1]["pose"])          # not observed: untouched
    capsys.readouterr()
    _run_tool("reoptimise_map.py", ["--config", cfg_path, "--map_dir", str(map_dir), "--gpus", "1", "--tol", str(TOL[0]), str(TOL[1])])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("iterations used: ")]
    assert line == ["iterations used: " + R.iterations_histogram(used)], (text, used)
    vals, cnt = np.unique(used, return_counts=True)
    assert "mean %.2f over 5 objects" % used.mean() in line[0] and all("%d: %d" % (v, c) in line[0] for v, c in zip(vals, cnt))
    # without the flag the tool prints no such line
    _run_tool("reoptimise_map.py", ["--config", cfg_path, "--map_dir", str(map_dir), "--gpus", "1"])
    assert "iterations used" not in capsys.readouterr().out
