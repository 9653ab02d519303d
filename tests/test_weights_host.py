"""CPU tier of the per-observation weights (dsp_batch_observation_weights, include/dsp_gn.h): bindings, argument checks, keyword plumbing,
observations.reject, and the weighted fp64 reference (tests/weights_ref.py) that tests/test_gpu_weights.py holds the device to."""
import ctypes as C
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

import multiview_metric as X
import multiview_oracle as MV
import weights_ref as W
from conftest import ROOT, golden
from dsp_slam_amd import _lib as L, engine as E, observations as OBS
from oracle import dsp_oracle as O
from test_gn_metric import _state

F32 = np.float32


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_bindings_and_header():
    bound = {n: (r, a) for n, r, a in L.SYMBOLS}
    assert bound["dsp_batch_observation_weights"] == (C.c_int, [C.c_void_p, L.c_f32p, L.c_f32p])
    assert bound["dsp_debug_observation_weights_check"] == (C.c_int, [C.c_int64, C.c_int64, L.c_f32p, L.c_f32p])
    hdr = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    assert re.search(r"int dsp_batch_observation_weights\(dsp_batch\* b, const float\* pt_w, const float\* ray_w\);", hdr)
    assert re.search(r"int dsp_debug_observation_weights_check\(int64_t n_points, int64_t n_rays, const float\* pt_w, const float\* ray_w\);", hdr)
    lib = L.load()
    assert hasattr(lib, "dsp_batch_observation_weights") and hasattr(lib, "dsp_debug_observation_weights_check")
    assert lib.dsp_abi_version() == L.ABI_VERSION == 6
    setters = sorted(n for n in bound if n.startswith("dsp_batch_set_"))
    assert setters == ["dsp_batch_set_compute", "dsp_batch_set_debug", "dsp_batch_set_iterations", "dsp_batch_set_kernel_timing", "dsp_batch_set_prepass",
                       "dsp_batch_set_prepass_guard", "dsp_batch_set_ray_passes"]
    assert not re.search(r"dsp_batch_set_\w*weight", hdr)
    assert lib.dsp_batch_observation_weights(None, None, None) == -1          # a stale token: DSP_E_ARG
    one = np.ones(3, F32)
    assert lib.dsp_batch_observation_weights(None, L.ptr(one), L.ptr(one)) == -1
    assert callable(E.Batch.set_observation_weights) and E.MultiviewBatch.set_observation_weights is E.Batch.set_observation_weights


def _check(pt_w, ray_w, n_p=None, n_r=None):
    pw = None if pt_w is None else np.ascontiguousarray(pt_w, F32)
    rw = None if ray_w is None else np.ascontiguousarray(ray_w, F32)
    n_p = (0 if pw is None else pw.size) if n_p is None else n_p
    n_r = (0 if rw is None else rw.size) if n_r is None else n_r
    return L.load().dsp_debug_observation_weights_check(n_p, n_r, L.ptr(pw), L.ptr(rw))


def test_argument_checks():
    ok = [1.0, 0.0, 0.25, 4.0, 1e-30, 3e38]
    assert _check(ok, ok) == 0
    assert _check(None, None, 5, 7) == 0 and _check(ok, None, n_r=9) == 0 and _check(None, ok, n_p=9) == 0      # NULL = all ones
    assert _check(np.zeros(4), np.zeros(3)) == 0                                 # all zero is a valid setting: the object then fails
    for bad in (-1.0, -0.0 - 1e-30, np.nan, np.inf, -np.inf):
        for pos in (0, 5):
            w = np.array(ok, F32)
            w[pos] = bad
            assert _check(w, ok) == -1, bad
            assert _check(ok, w) == -1, bad
            assert _check(w, None, n_r=4) == -1 and _check(None, w, n_p=4) == -1
    assert _check([-0.0], [-0.0]) == 0                                           # -0 is zero
    assert _check(None, None, -1, 0) == -1 and _check(None, None, 0, -1) == -1


# ---- Python plumbing -------------------------------------------------------------------------------------------------------------------
def test_engine_keyword_sits_in_front_of_report():
    for fn in (E.Engine.reconstruct_batch, E.Engine.reconstruct_multiview_batch, E.Engine.estimate_pose_batch):
        p = inspect.signature(fn).parameters
        assert list(p)[-3:] == ["obs_weights", "report", "prior"] and p["obs_weights"].default is None
    p = inspect.signature(E._run_resident).parameters
    assert list(p)[-1] == "obs_weights" and p["obs_weights"].default is None
    assert list(inspect.signature(E.Batch.set_observation_weights).parameters) == ["self", "pt_w", "ray_w"]


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


def test_optimizer_keyword_sits_in_front_of_prior(mirror):
    from reconstruct.optimizer import Optimizer
    from reconstruct.utils import ForceKeyErrorDict
    for fn in (Optimizer.reconstruct_object, Optimizer.reconstruct_object_multiview, Optimizer.estimate_pose_cam_obj):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["obs_weights", "prior"] and p["obs_weights"].default is None
    for fn in (Optimizer.reconstruct_objects, Optimizer.estimate_poses_cam_obj):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["obs_weights", "priors"] and p["obs_weights"].default is None

    class FakeEngine(object):
        def reconstruct_batch(self, prm, t, pts, rays, depth, codes=None, **kw):
            self.kw = kw
            n = len(pts)
            return (np.tile(np.eye(4, dtype=F32), (n, 1, 1)), np.zeros((n, 64), F32), np.zeros(n, F32), np.zeros(n, np.int32))

        def estimate_pose_batch(self, prm, t, scale, pts, codes, **kw):
            self.kw = kw
            return np.tile(np.eye(4, dtype=F32), (len(pts), 1, 1))
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    cfg.setdefault("data_type", "KITTI")
    opt = Optimizer(None, ForceKeyErrorDict(cfg))
    opt.verbose = False
    eng = FakeEngine()
    opt.decoder = type("D", (), {"engine": eng})()
    pts, rays, depth = np.zeros((4, 3), F32), np.zeros((6, 3), F32), np.zeros(4, F32)
    plain = opt.reconstruct_object(np.eye(4, dtype=F32), pts, rays, depth)
    assert "obs_weights" not in eng.kw and sorted(plain.keys()) == ["code", "is_good", "loss", "t_cam_obj"]
    got = opt.reconstruct_object(np.eye(4, dtype=F32), pts, rays, depth, obs_weights=(np.arange(4), None))
    assert sorted(got.keys()) == ["code", "is_good", "loss", "t_cam_obj"]         # results keep the reference's four keys
    pw, rw = eng.kw["obs_weights"]
    assert pw[0].tolist() == [0, 1, 2, 3] and pw[0].dtype == F32 and rw[0].tolist() == [1] * 6
    opt.reconstruct_objects([np.eye(4, dtype=F32)] * 2, [pts] * 2, [rays] * 2, [depth] * 2, obs_weights=[None, (None, np.zeros(6))])
    pw, rw = eng.kw["obs_weights"]
    assert pw[0].tolist() == [1] * 4 and pw[1].tolist() == [1] * 4 and rw[0].tolist() == [1] * 6 and rw[1].tolist() == [0] * 6
    import torch
    assert isinstance(opt.estimate_pose_cam_obj(np.eye(4, dtype=F32), 1.0, pts, np.zeros(64, F32)), torch.Tensor) and "obs_weights" not in eng.kw
    assert isinstance(opt.estimate_pose_cam_obj(np.eye(4, dtype=F32), 1.0, pts, np.zeros(64, F32), obs_weights=(np.ones(4), None)), torch.Tensor)
    assert eng.kw["obs_weights"][1] is None and eng.kw["obs_weights"][0][0].tolist() == [1] * 4


def test_run_resident_sets_the_weights_in_front_of_the_run():
    class FakeBatch(object):
        def __init__(self):
            self.calls = []

        def set_report(self, on):
            self.calls.append(("report", on))

        def set_observation_weights(self, pt_w=None, ray_w=None):
            self.calls.append(("weights", pt_w, ray_w))

        def run(self):
            self.calls.append(("run",))

        def results(self):
            return (1, 2, 3, 4)

        def report(self):
            return "rep"
    b = FakeBatch()
    assert E._run_resident(b, None, None, None) == (1, 2, 3, 4) and b.calls == [("run",)]          # None: no call on the batch
    b = FakeBatch()
    assert E._run_resident(b, None, None, None, None, None, ("p", "r")) == (1, 2, 3, 4) and b.calls == [("weights", "p", "r"), ("run",)]
    b = FakeBatch()
    assert E._run_resident(b, None, None, None, None, True, ("p", None)) == (1, 2, 3, 4, "rep")
    assert b.calls == [("report", True), ("weights", "p", None), ("run",)]


def test_reject():
    nan = np.nan
    rep = dict(pt_sdf=np.array([0.0, 0.02, -0.03, 0.011, nan, 0.001], F32), pt_alive=np.array([1, 1, 1, 1, 0, 0], bool),
               ray_residual=np.array([0.0, 0.1, -0.11, nan, 0.0999, -5.0], F32))
    pt_w, ray_w = OBS.reject(rep, 0.02, 0.1)
    assert pt_w.dtype == F32 and ray_w.dtype == F32
    assert pt_w.tolist() == [1, 1, 0, 1, 0, 0]          # the bound itself passes; a dead or unevaluated point gets 0
    assert ray_w.tolist() == [1, 1, 0, 1, 1, 0]         # a ray whose row is NaN keeps 1
    assert _check(pt_w, ray_w) == 0


def test_tool_flag():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import reoptimise_map as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    p = inspect.signature(tool.reoptimise).parameters
    assert "reject" in p and p["reject"].default is None
    src = open(os.path.join(ROOT, "tools", "reoptimise_map.py")).read()
    assert '"--reject"' in src and "PT_SDF" in src and "set_observation_weights" in src


# ---- the weighted fp64 reference -------------------------------------------------------------------------------------------------------
KEYS = ("H", "b", "dx", "Dr", "Ds", "gr", "gs", "Lr", "Ls", "H_code_prior", "b_code_prior", "H_rot", "b_rot", "H_damp", "H_flip", "b_flip")


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= rel * max(np.abs(b).max(), 1e-300)))


@pytest.mark.parametrize("name", ["golden_recon_small.npz", "golden_recon_redwood.npz"])
def test_unit_weights_reproduce_linearise_fp64(name):
    prm, dec, inputs, state, ref, it, lin = _state(name, 0)
    for pw, rw in ((None, None), (np.ones(inputs[0].shape[0], F32), np.ones(inputs[1].shape[0], F32))):
        got = W.linearise(dec, prm, *inputs, *state, it["sets"], pw, rw)
        for k in KEYS:
            assert _close(got[k], lin[k]), k
        assert (got["V"], got["K"], got["N"]) == (lin["V"], lin["K"], lin["N"]) and got["Mw"] == lin["N"] and got["Kw"] == lin["K"]


def test_unit_weights_reproduce_the_pooled_fp64_of_the_recorded_three_view_run(oracle_decoder):
    g = golden("golden_multiview_cars3.npz")
    prm = O.GNParams.from_configs(json.loads(str(g["cfg_json"])))
    views = MV.golden_views(g)
    e = 0
    it, _, lin = X.linearise_at(oracle_decoder, prm, views, g["it_t_obj_cam"][e], g["it_code"][e], g["it_depths"][e])
    depths, sets = [v["depths"] for v in it["views"]], [v["sets"] for v in it["views"]]
    ones = ([np.ones(v["pts"].shape[0], F32) for v in views], [np.ones(v["rays"].shape[0], F32) for v in views])
    for pw, rw in ((None, None), ones):
        got = W.linearise_multiview(oracle_decoder, prm, views, g["it_t_obj_cam"][e], g["it_code"][e], depths, sets, pw, rw)
        for k in KEYS:
            assert _close(got[k], lin[k]), k
        assert got["K_views"] == lin["K_views"] and got["Mw"] == lin["N"] and got["Kw"] == lin["K"]


def _random_rows(rng, n_s, n_k, n=71):
    j_s, j_r = rng.normal(size=(n_s, n)), rng.normal(size=(n_k, n))
    return dict(j_s=j_s, j_s2=j_s.copy(), r_s=rng.normal(size=n_s) * 0.01, j_r=j_r, j_r2=j_r.copy(), r_r=rng.normal(size=n_k) * 0.1, V=3 * n_k, K=n_k, N=n_s)


def test_weighted_assembly_against_a_brute_force_sum():
    """Two views, weights in [0.1, 4] with exact zeros, one view's rays all zero: the data terms are the plain weighted sums over the
    pooled weight sums; priors and damping are those of the unweighted system; H, b and dx put them together."""
    rng = np.random.default_rng(5)
    prm = O.GNParams(num_iterations=1, **X.HYPER)
    rows = [_random_rows(rng, 23, 17), _random_rows(rng, 9, 11)]
    w = [(rng.uniform(0.1, 4, 23), rng.uniform(0.1, 4, 17)), (rng.uniform(0.1, 4, 9), np.zeros(11))]
    w[0][0][::5] = 0.0
    w[0][1][3] = 0.0
    t = np.eye(4, dtype=F32)
    t[:3, :3] = 0.5 * np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], F32)
    code = rng.normal(size=64).astype(F32) * 0.1
    got = W.assemble(prm, rows, w, t, code)
    ds, gs, ls, dr, gr, lr = W.brute_force(prm, rows, w, code)
    for a, b, k in ((got["Ds"], ds, "Ds"), (got["gs"], gs, "gs"), (got["Ls"], ls, "Ls"), (got["Dr"], dr, "Dr"), (got["gr"], gr, "gr"), (got["Lr"], lr, "Lr")):
        assert _close(a, b, 1e-11), k
    plain = O._assemble64(prm, rows, t, code)
    for k in ("H_code_prior", "b_code_prior", "H_rot", "b_rot", "H_damp"):
        assert np.array_equal(got[k], plain[k]), k
    assert _close(got["H"], dr + ds + got["H_code_prior"] + got["H_rot"] + got["H_damp"], 1e-11)
    assert _close(got["b"], gr + gs + got["b_code_prior"] + got["b_rot"], 1e-11)
    assert _close(got["H"] @ got["dx"], got["b"], 1e-9)
    assert abs(got["Mw"] - (w[0][0].sum() + w[1][0].sum())) < 1e-12 and abs(got["Kw"] - w[0][1].sum()) < 1e-12
    assert (got["N"], got["K"]) == (32, 28)                                      # counts stay counts
    # a weight that doubles everywhere changes nothing: the sums normalise
    twice = W.assemble(prm, rows, [(2 * a, 2 * b) for a, b in w], t, code)
    assert _close(twice["H"], got["H"], 1e-12) and _close(twice["b"], got["b"], 1e-12)


def test_row_weights_follow_the_kept_rows_ray():
    sets = dict(valid=(np.zeros(0, np.int64),) * 2, kept=(np.array([4, 4, 0, 2]), np.array([1, 2, 7, 3])))
    w_s, w_r = W.row_weights(sets, None, np.array([0.5, 9, 2.0, 9, 0.25], F32), 3)
    assert w_s.tolist() == [1, 1, 1] and w_r.tolist() == [0.25, 0.25, 0.5, 2.0]
