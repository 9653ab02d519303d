"""GPU: the pose-only optimiser beyond five iterations -- the inlier filter after the update of e == 4 and the changed 1 / M of the
iterations after it (reference optimizer.py:59-78) -- against tests/golden/golden_pose_only_8it.npz (tools/make_golden.py pose8), and
objects that the filter leaves without points, or that have none: the reference returns NaN for them.

The batch is the one dsp_estimate_pose_batch runs, made resident by dsp_batch_create_pose so that it can be traced; its trace carries, in
K, the number of points each iteration's system was built from.
"""
import json
import os

import numpy as np
import pytest

from conftest import golden, parity_log
from oracle import dsp_oracle as O
from dsp_slam_amd import engine as E

pytestmark = pytest.mark.gpu

TOL = 1e-4


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _prm(n_it):
    return E.gn_params(pose_only_iterations=n_it)


def _objects():
    """(t_co_se3, scale, pts, code) of: the 8-iteration golden's object, a clean object the filter leaves whole, the all-outlier object,
    golden_pose_only.npz's object."""
    g, g5 = golden("golden_pose_only_8it.npz"), golden("golden_pose_only.npz")
    clean = g5["pts"][:200]
    return [(g["t_co_se3"], float(g["scale"]), g["pts"], g["code"]),
            (g5["t_co_se3"], float(g5["scale"]), clean, g5["code"]),
            (g["allout_t_co_se3"], float(g["allout_scale"]), g["allout_pts"], g["allout_code"]),
            (g5["t_co_se3"], float(g5["scale"]), g5["pts"], g5["code"])]


def _batch(eng, objs, n_it, trace=False):
    return eng.pose_batch(_prm(n_it), [o[0] for o in objs], [o[1] for o in objs], [o[2] for o in objs], [o[3] for o in objs], trace=trace)


def _run(b):
    b.run()
    t, _, _, status = b.results()
    return t, status


def test_chained_eight_iterations_against_the_reference(eng):
    """The device chained from the golden's input: the point count of every iteration exactly, and the state each iteration starts from,
    and the output, within 1e-4.  The chained H / b are reported, not held to 1e-4: on this golden a state one ulp away flips a hidden
    ReLU of one point and moves H by 2e-4 at iteration 5 (the CPU oracle shows the same, tests/test_oracle_golden.py) -- the per-iteration
    systems are compared at the reference's own states below."""
    g = golden("golden_pose_only_8it.npz")
    b = _batch(eng, _objects()[:1], 8, trace=True)
    t, status = _run(b)
    tr = [b.trace(e) for e in range(8)]
    b.close()
    assert status[0] == 0
    assert [int(x["K"][0]) for x in tr] == list(g["it_n"]), [int(x["K"][0]) for x in tr]
    for e, x in enumerate(tr):
        assert rel(x["t_obj_cam"][0], g["it_t_obj_cam"][e]) < TOL, e
    assert rel(t[0], g["out"]) < TOL
    parity_log(kind="pose_only_chained", case="golden_pose_only_8it.npz", alive=[int(x["K"][0]) for x in tr], alive_ref=[int(n) for n in g["it_n"]],
               rel_H=[rel(x["H"][0], g["it_H"][e]) for e, x in enumerate(tr)], rel_b=[rel(x["b"][0], g["it_b"][e]) for e, x in enumerate(tr)],
               rel_out=rel(t[0], g["out"]))


def test_every_iteration_at_the_reference_states(eng):
    """Each of the 8 iterations linearised at the reference's recorded camera->object matrix (injected bit for bit) on the points the
    reference's system used (all of them before the filter, the recorded survivors after): H, b, dx within 1e-4 relative, the count exact."""
    g = golden("golden_pose_only_8it.npz")
    rows = []
    for e in range(8):
        pts = g["pts"] if e < 5 else g["pts"][g["mask_e4"]]
        b = eng.pose_batch(_prm(1), [g["t_co_se3"]], [float(g["scale"])], [pts], [g["code"]], trace=True)
        b.set_start_state([g["it_t_obj_cam"][e]])
        t, status = _run(b)
        x = b.trace(0)
        b.close()
        assert status[0] == 0
        assert np.array_equal(x["t_obj_cam"][0], g["it_t_obj_cam"][e])
        assert int(x["K"][0]) == int(g["it_n"][e])
        r = dict(H=rel(x["H"][0], g["it_H"][e]), b=rel(x["b"][0], g["it_b"][e]), dx=rel(x["dx"][0], g["it_dx"][e]))
        rows.append(r)
        assert r["H"] < TOL and r["b"] < TOL and r["dx"] < TOL, (e, r)
    print("pose-only at the reference's states: largest rel dH / db at iterations 5-7: %.2e / %.2e" % (
        max(r["H"] for r in rows[5:]), max(r["b"] for r in rows[5:])))
    parity_log(kind="pose_only_at_reference_states", case="golden_pose_only_8it.npz", rel_H=[r["H"] for r in rows],
               rel_b=[r["b"] for r in rows], rel_dx=[r["dx"] for r in rows])


def test_ragged_batch_with_an_object_the_filter_empties(eng):
    """Four objects in one batch -- the 8-iteration golden's, a clean one that keeps all its points, one whose every point the filter
    drops, and golden_pose_only.npz's: each result equals its single-object run bit for bit; the first is the reference's, the emptied
    one is NaN like the reference's (not the last finite state), its status DSP_OBJ_NAN; the others are unaffected."""
    g = golden("golden_pose_only_8it.npz")
    objs = _objects()
    b = _batch(eng, objs, 8, trace=True)
    t, status = _run(b)
    counts = [b.trace(e)["K"] for e in range(5)] + [b.trace(5)["K"]]
    b.close()
    for i, o in enumerate(objs):
        b1 = _batch(eng, [o], 8)
        t1, s1 = _run(b1)
        b1.close()
        assert s1[0] == status[i]
        assert np.array_equal(t1[0], t[i], equal_nan=True), i
        # ... and the one-shot entry point returns the same bits
        assert np.array_equal(eng.estimate_pose_batch(_prm(8), [o[0]], [o[1]], [o[2]], [o[3]])[0], t[i], equal_nan=True), i
    assert rel(t[0], g["out"]) < TOL
    assert list(status) == [0, 0, 2, 0]
    assert np.isnan(t[2]).all() and np.isnan(g["allout_out"]).all()
    assert np.isfinite(t[[0, 1, 3]]).all()
    assert [int(c[1]) for c in counts] == [200] * 6                       # the clean object keeps every point
    assert [int(c[2]) for c in counts] == list(g["allout_it_n"][:6])      # 150 x 5, then 0
    assert [int(c[0]) for c in counts] == list(g["it_n"][:6])


def test_an_object_without_points(eng):
    """No points at all: the reference's pose is NaN (recorded); so is the device's, alone and next to a regular object."""
    g = golden("golden_pose_only_8it.npz")
    assert np.isnan(g["empty_out"]).all()
    empty = (g["t_co_se3"], float(g["scale"]), np.zeros((0, 3), np.float32), g["code"])
    for n_it in (8, 5):
        b = _batch(eng, [empty, _objects()[3]], n_it)
        t, status = _run(b)
        b.close()
        assert list(status) == [2, 0] and np.isnan(t[0]).all() and np.isfinite(t[1]).all(), n_it


def test_iteration_counts_on_one_batch(eng):
    """set_iterations 5, 6, 8, 10 and 5 again on ONE batch: every run equals a fresh batch's run bit for bit (the filter's mask and count
    are reset per run), the recorded reference outputs are met, and 5 iterations are dsp_estimate_pose_batch's golden_pose_only.npz result."""
    g = golden("golden_pose_only_8it.npz")
    objs = _objects()
    b = _batch(eng, objs, 5)
    for n_it in (5, 6, 8, 10, 5):
        b.set_iterations(n_it)
        t, status = _run(b)
        f = _batch(eng, objs, n_it)
        t1, s1 = _run(f)
        f.close()
        assert np.array_equal(t, t1, equal_nan=True) and np.array_equal(status, s1), n_it
        ref = g["out"] if n_it == 8 else g["out_%dit" % n_it]
        assert rel(t[0], ref) < TOL, (n_it, rel(t[0], ref))
        assert (status[2] == 2) == (n_it > 5)
        if n_it == 5:
            g5 = golden("golden_pose_only.npz")
            one = eng.estimate_pose_batch(_prm(5), [g5["t_co_se3"]], [float(g5["scale"])], [g5["pts"]], [g5["code"]])
            assert np.array_equal(one[0], t[3])
            assert rel(t[3], g5["out"]) < TOL
    b.close()


def test_mirror_with_eight_pose_only_iterations(cars_state_dict, tmp_path):
    """The Python mirror's Optimizer.estimate_pose_cam_obj under a config whose pose_only_optim.num_iterations is 8."""
    import sys
    from dsp_slam_amd import fixtures
    g = golden("golden_pose_only_8it.npz")
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsp_slam_amd")
    sys.path.insert(0, pkg)
    try:
        for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
            del sys.modules[m]
        from reconstruct.utils import get_configs, get_decoder
        from reconstruct.optimizer import Optimizer
        cfg_d = json.loads(str(g["cfg_json"]))
        assert cfg_d["optimizer"]["pose_only_optim"]["num_iterations"] == 8
        cfg_d["DeepSDF_DIR"] = fixtures.materialize_decoder_dir("cars", str(tmp_path / "cars_64"))
        with open(tmp_path / "cfg.json", "w") as f:
            json.dump(cfg_d, f)
        cfg = get_configs(str(tmp_path / "cfg.json"))
        opt = Optimizer(get_decoder(cfg), cfg)
        opt.verbose = False
        out = opt.estimate_pose_cam_obj(g["t_co_se3"].copy(), float(g["scale"]), g["pts"], g["code"])
        assert rel(out.numpy(), g["out"]) < TOL
        out = opt.estimate_pose_cam_obj(g["allout_t_co_se3"].copy(), float(g["allout_scale"]), g["allout_pts"], g["allout_code"])
        assert np.isnan(out.numpy()).all()
    finally:
        sys.path.remove(pkg)
        for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
            del sys.modules[m]
