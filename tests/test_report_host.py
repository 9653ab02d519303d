"""CPU-only: the observation report (dsp_batch_report, include/dsp_gn.h) above and below the device.

  * the per-ray arithmetic: dsp_debug_report_ray (csrc/report_math.h, the scalar function the device kernels are built from) against the
    chain written sequentially in float32 (tests/report_ref.py: chain_ray) -- bit equality of the four floats, equality of the counts -- on
    random rows at num_depth_samples 2, 50 and 64, an empty row, a full row, a first-sample hit and a NaN observed depth;
  * the restatement from oracle pieces agrees with the sequential chain to its own tolerance (it sums in another order);
  * dsp_slam_amd.observations on hand-made reports;
  * plumbing: bindings, the `report` keyword (position and default), the Optimizer keys through a fake engine, the tool's flag.
"""
import copy
import inspect
import json
import os
import sys

import numpy as np
import pytest

import report_ref as R
from conftest import ROOT
from dsp_slam_amd import _lib as L, engine as E, observations as OBS

F32 = np.float32


def _device_ray(depths, sdf, th, depth_obs, is_fg):
    d, s = L.f32(depths), L.f32(sdf)
    out4, c3 = np.zeros(4, F32), np.zeros(3, np.int32)
    rc = L.load().dsp_debug_report_ray(d.shape[0], L.ptr(d), L.ptr(s), float(th), float(depth_obs), int(is_fg), L.ptr(out4), L.ptr(c3, L.c_i32p))
    assert rc == 0
    return out4, c3


def _random_row(rng, n_depth, th, p_in=0.6):
    """Depth samples as an iteration derives them, and an sdf row that crosses the band: outside (NaN), free space, band, solid."""
    d0 = rng.uniform(4.0, 20.0)
    depths = np.linspace(d0, d0 + rng.uniform(2.0, 4.4), n_depth).astype(F32)
    kind = rng.choice(4, size=n_depth, p=[1.0 - p_in, p_in * 0.5, p_in * 0.3, p_in * 0.2])
    sdf = np.where(kind == 0, np.nan, np.where(kind == 1, rng.uniform(th, 0.3, n_depth), np.where(kind == 2, rng.uniform(-th, th, n_depth),
                                                                                                   rng.uniform(-0.2, -th, n_depth)))).astype(F32)
    return depths, sdf


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


@pytest.mark.parametrize("n_depth", [2, 50, 64])
def test_ray_arithmetic_is_the_sequential_chain_bit_for_bit(n_depth):
    rng = np.random.default_rng(900 + n_depth)
    th = 0.01
    rows = [_random_row(rng, n_depth, th) for _ in range(200)]
    rows += [_random_row(rng, n_depth, th, p_in=1.0) for _ in range(20)]                # full rows
    d, s = _random_row(rng, n_depth, th)
    rows.append((d, np.full(n_depth, np.nan, F32)))                                      # an empty row
    s_hit = s.copy()
    s_hit[0] = F32(-0.5)                                                                 # a first-sample hit: T = 0 from the first sample on
    rows.append((d, s_hit))
    s_edge = np.where(np.arange(n_depth) % 2 == 0, F32(th), F32(-th)).astype(F32)        # exactly on the thresholds: not in the band
    rows.append((d, s_edge))
    n_kept = 0
    for i, (depths, sdf) in enumerate(rows):
        for is_fg, obs in ((1, float(depths[n_depth // 2]) + 0.01 * (i % 7)), (0, 0.0), (1, float("nan"))):
            got4, got3 = _device_ray(depths, sdf, th, obs, is_fg)
            ref4, ref3 = R.chain_ray(depths, sdf, th, obs, is_fg)
            assert _same_bits(got4, ref4), (n_depth, i, is_fg, got4, ref4)
            assert got3.tolist() == ref3.tolist(), (n_depth, i, got3, ref3)
            if np.isnan(obs) and is_fg:
                assert np.isnan(got4[2]) and np.isnan(got4[3]) and not np.isnan(got4[0])   # a NaN observed depth stays NaN through the clip
            n_kept += int(got3[2])
    assert n_kept > 50          # the rows do exercise the keep test
    # the empty row renders the background; the first-sample hit renders its first depth and terminates everything behind it
    d4, c3 = _device_ray(d, np.full(n_depth, np.nan, F32), th, 0.0, 0)
    assert c3.tolist() == [0, 0, 0] and d4[1] == 0.0 and d4[0] == F32(F32(1.1) * d[-1]) and d4[2] == 0.0
    d4, c3 = _device_ray(d, s_hit, th, float(d[0]), 1)
    assert d4[1] == 1.0 and d4[0] == d[0] and d4[2] == 0.0


def test_a_sample_behind_a_terminating_sample_contributes_exactly_zero():
    """T = 0 behind a solid sample: whatever finite value the samples behind it hold -- the placeholder of a sample that was never decoded --
    the ray's floats and its kept count are the same bits."""
    rng = np.random.default_rng(5)
    depths, sdf = _random_row(rng, 50, 0.01, p_in=1.0)
    sdf[10] = F32(-0.3)
    a4, a3 = _device_ray(depths, sdf, 0.01, float(depths[10]), 1)
    other = sdf.copy()
    other[11:] = F32(1.0)
    b4, b3 = _device_ray(depths, other, 0.01, float(depths[10]), 1)
    assert _same_bits(a4, b4) and a3[2] == b3[2] and a3[0] == b3[0]
    assert not np.isnan(a4).any()


def test_ray_argument_checks():
    lib = L.load()
    d, s, o, c = np.ones(70, F32), np.zeros(70, F32), np.zeros(4, F32), np.zeros(3, np.int32)
    for n in (1, 65):
        assert lib.dsp_debug_report_ray(n, L.ptr(d), L.ptr(s), 0.01, 0.0, 0, L.ptr(o), L.ptr(c, L.c_i32p)) == -1
    assert lib.dsp_debug_report_ray(50, L.ptr(d), L.ptr(s), 0.0, 0.0, 0, L.ptr(o), L.ptr(c, L.c_i32p)) == -1
    assert lib.dsp_debug_report_ray(50, None, L.ptr(s), 0.01, 0.0, 0, L.ptr(o), L.ptr(c, L.c_i32p)) == -1


def test_oracle_restatement_agrees_with_the_chain(oracle_decoder):
    """report_ref.evaluate32 (numpy's cumprod / sum) and the sequential chain on the same sdf grid: same counts, floats within the bounds."""
    from oracle import dsp_oracle as O
    o = R.joint_objects()[0]
    prm = R.oracle_params(50)
    t_oc = O._inv(o["t_cam_obj_gt"])
    depths = R.derived_depths(t_oc, 50)
    r = R.evaluate32(oracle_decoder, prm, o["pts"], o["rays"], o["depth"], t_oc, o["code_gt"], depths)
    assert r["V"] >= 10 and r["K"] > 0 and r["M"] == 120
    n_fg = o["depth"].shape[0]
    for i in range(o["rays"].shape[0]):
        got4, got3 = R.chain_ray(depths, r["sdf_grid"][i], prm.cut_off, o["depth"][i] if i < n_fg else 0.0, i < n_fg)
        assert got3.tolist() == r["ray_counts"][i].tolist()
        for k, f in enumerate(("ray_depth", "ray_hit", "ray_residual")):
            assert abs(float(got4[k]) - float(r[f][i])) <= R.bound(f, r[f][i]), (i, f)


# ---- observations.py on hand-made reports -------------------------------------------------------------------------------------------------
def _hand_report():
    """Two objects: the first with two views (members 0, 1), the second with one (member 2), which failed."""
    nan = np.nan
    return dict(
        pt_sdf=np.array([0.001, -0.03, 0.02, 0.0, 0.004, nan, nan], F32), pt_alive=np.array([1, 1, 0, 1, 1, 0, 0], bool),
        pt_flags=np.array([1, 1, 0, 1, 1, 0, 0], np.uint8),
        ray_depth=np.zeros(7, F32), ray_residual=np.zeros(7, F32), ray_counts=np.zeros((7, 3), np.int32),
        ray_hit=np.array([0.9, 0.2, 0.7, 0.6, 0.1, nan, nan], F32),
        M=np.array([3, 2, 0]), V=np.array([40, 30, 0]), m=np.array([5, 4, 0]), K=np.array([4, 0, 0]),
        sum_s=np.array([0.03, 0.002, nan]), sum_r=np.array([0.4, 0.0, nan]), status=np.array([0, 0, 1], np.int32),
        pts_off=np.array([0, 3, 5, 7]), ray_off=np.array([0, 4, 5, 7]), depth_off=np.array([0, 2, 2, 3]), view_off=np.array([0, 2, 3]))


def test_point_outliers():
    masks = OBS.point_outliers(_hand_report(), 0.01)
    assert [m.tolist() for m in masks] == [[False, True, True], [False, False], [True, True]]      # |sdf| > tol, a dead point, NaN rows
    assert [m.tolist() for m in OBS.point_outliers(_hand_report(), 1.0)] == [[False, False, True], [False, False], [True, True]]


def test_view_scores():
    prm = E.gn_params(k1=2.0, k2=100.0)
    out = OBS.view_scores(_hand_report(), prm)
    s0, s1 = 100.0 * 0.03 / 3 + 2.0 * 0.4 / 4, 100.0 * 0.002 / 2          # K = 0: no render term
    assert np.allclose(out["score"][:2], [s0, s1], rtol=1e-12) and np.isnan(out["score"][2])
    med = 0.5 * (s0 + s1)
    assert np.allclose(out["ratio"][:2], [s0 / med, s1 / med], rtol=1e-12) and np.isnan(out["ratio"][2])
    assert np.allclose(OBS.view_scores(_hand_report(), dict(k1=2.0, k2=100.0))["score"][:2], [s0, s1])


def test_silhouette_disagreement():
    rep = _hand_report()
    out = OBS.silhouette_disagreement(rep)
    # member 0: foreground hits 0.9, 0.2 -> one of two below 0.5; background 0.7, 0.6 -> both above.  member 1: no foreground ray, one background ray at 0.1
    assert out["fg_miss"][0] == 0.5 and out["bg_hit"][0] == 1.0
    assert np.isnan(out["fg_miss"][1]) and out["bg_hit"][1] == 0.0
    assert np.isnan(out["fg_miss"][2]) and np.isnan(out["bg_hit"][2])
    out = OBS.silhouette_disagreement(rep, n_fg=[4, 1, 1])
    assert out["fg_miss"][0] == 0.25 and np.isnan(out["bg_hit"][0]) and out["fg_miss"][1] == 1.0


def test_object_rows():
    rep = _hand_report()
    a, b = OBS.object_rows(rep, 0), OBS.object_rows(rep, 1)
    assert a["pt_sdf"].shape == (5,) and a["ray_hit"].shape == (5,) and a["M"].tolist() == [3, 2] and a["pts_off"].tolist() == [0, 3, 5]
    assert a["ray_off"].tolist() == [0, 4, 5] and a["depth_off"].tolist() == [0, 2, 2] and a["view_off"].tolist() == [0, 2]
    assert b["pt_sdf"].shape == (2,) and b["status"].tolist() == [1] and b["pts_off"].tolist() == [0, 2] and b["ray_off"].tolist() == [0, 2]
    assert [m.tolist() for m in OBS.point_outliers(a, 0.01)] == [[False, True, True], [False, False]]


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def test_bindings():
    import ctypes as C
    bound = {n: (r, a) for n, r, a in L.SYMBOLS}
    assert bound["dsp_batch_report"][1] == [C.c_void_p, C.c_int]
    assert len(bound["dsp_batch_report_sizes"][1]) == 4 and len(bound["dsp_batch_report_fetch"][1]) == 8 and len(bound["dsp_debug_report_ray"][1]) == 8
    lib = L.load()
    for n in ("dsp_batch_report", "dsp_batch_report_sizes", "dsp_batch_report_fetch", "dsp_debug_report_ray"):
        assert hasattr(lib, n)
    assert lib.dsp_abi_version() == 6
    assert not [n for n in bound if n.startswith("dsp_batch_set_report")]
    assert callable(E.Batch.set_report) and callable(E.Batch.report) and E.MultiviewBatch.report is E.Batch.report
    assert lib.dsp_batch_report(None, 1) == -1 and lib.dsp_batch_report_fetch(None, *([None] * 7)) == -1      # a stale token: DSP_E_ARG


def test_report_keyword_sits_in_front_of_prior():
    for fn in (E.Engine.reconstruct_batch, E.Engine.reconstruct_multiview_batch, E.Engine.estimate_pose_batch):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["report", "prior"] and inspect.signature(fn).parameters["report"].default is None


def test_run_resident_returns_the_report_behind_the_posterior():
    class FakeBatch(object):
        def __init__(self):
            self.calls = []

        def set_report(self, on):
            self.calls.append(("report", on))

        def set_posterior(self, *a):
            self.calls.append(("posterior",) + a)

        def set_prior(self, *a):
            self.calls.append(("prior",))

        def run(self):
            self.calls.append(("run",))

        def results(self):
            return (1, 2, 3, 4)

        def posterior(self):
            return "post"

        def report(self):
            return "rep"

        def prior_residual(self):
            return "pri"
    b = FakeBatch()
    assert E._run_resident(b, None, None, None) == (1, 2, 3, 4) and b.calls == [("run",)]
    b = FakeBatch()
    assert E._run_resident(b, None, None, None, None, True) == (1, 2, 3, 4, "rep") and b.calls == [("report", True), ("run",)]
    assert E._run_resident(FakeBatch(), None, "mean", (0, 0, 0), None, True) == (1, 2, 3, 4, "post", "rep", "pri")
    assert E._run_resident(FakeBatch(), None, None, None, None, False) == (1, 2, 3, 4)


@pytest.fixture
def mirror():
    """The package directory on sys.path, as the drop-in layout has it (reconstruct.*, deep_sdf.* importable by those names)."""
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    sys.path.insert(0, pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    yield
    sys.path.remove(pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]


def test_optimizer_config_keys(mirror):
    """joint_optim.report / pose_only_optim.report: absent or false = off and the result is the reference's four keys; true goes to the
    Engine calls as report=True and good results carry `observations`."""
    from reconstruct.optimizer import Optimizer
    from reconstruct.utils import ForceKeyErrorDict
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    base.setdefault("data_type", "KITTI")

    def optimizer(joint=None, pose=None):
        cfg = copy.deepcopy(base)
        if joint is not None:
            cfg["optimizer"]["joint_optim"]["report"] = joint
        if pose is not None:
            cfg["optimizer"].setdefault("pose_only_optim", {"num_iterations": 5})["report"] = pose
        opt = Optimizer(None, ForceKeyErrorDict(cfg))
        opt.verbose = False
        return opt
    assert optimizer().report_joint is False and optimizer().report_pose_only is False and optimizer(False, False).report_joint is False
    assert optimizer(True).report_joint is True and optimizer(True).report_pose_only is False and optimizer(None, True).report_pose_only is True

    def fake_report(n):
        return dict(pt_sdf=np.zeros(4 * n, F32), pt_flags=np.ones(4 * n, np.uint8), pt_alive=np.ones(4 * n, bool), ray_depth=np.zeros(6 * n, F32),
                    ray_hit=np.zeros(6 * n, F32), ray_residual=np.zeros(6 * n, F32), ray_counts=np.zeros((6 * n, 3), np.int32),
                    M=np.full(n, 4), V=np.zeros(n, np.int64), m=np.zeros(n, np.int64), K=np.zeros(n, np.int64), sum_s=np.zeros(n), sum_r=np.zeros(n),
                    status=np.zeros(n, np.int32), pts_off=4 * np.arange(n + 1), ray_off=6 * np.arange(n + 1), depth_off=4 * np.arange(n + 1),
                    view_off=np.arange(n + 1))

    class FakeEngine(object):
        def reconstruct_batch(self, prm, t, pts, rays, depth, codes=None, **kw):
            self.kw = kw
            n = len(pts)
            res = (np.tile(np.eye(4, dtype=F32), (n, 1, 1)), np.zeros((n, 64), F32), np.zeros(n, F32), np.zeros(n, np.int32))
            return res + ((fake_report(n),) if kw.get("report") else ())

        def estimate_pose_batch(self, prm, t, scale, pts, codes, **kw):
            self.kw = kw
            n = len(pts)
            poses = np.tile(np.eye(4, dtype=F32), (n, 1, 1))
            return (poses, fake_report(n)) if kw.get("report") else poses
    eng = FakeEngine()
    pts, rays, depth = np.zeros((4, 3), F32), np.zeros((6, 3), F32), np.zeros(4, F32)
    opt = optimizer(True)
    opt.decoder = type("D", (), {"engine": eng})()
    two = opt.reconstruct_objects([np.eye(4, dtype=F32)] * 2, [pts] * 2, [rays] * 2, [depth] * 2)
    assert eng.kw["report"] is True and two[1].observations["pt_sdf"].shape == (4,) and two[1].observations["pts_off"].tolist() == [0, 4]
    opt = optimizer()
    opt.decoder = type("D", (), {"engine": eng})()
    plain = opt.reconstruct_object(np.eye(4, dtype=F32), pts, rays, depth)
    assert "report" not in eng.kw and sorted(plain.keys()) == ["code", "is_good", "loss", "t_cam_obj"]
    import torch
    assert isinstance(opt.estimate_pose_cam_obj(np.eye(4, dtype=F32), 1.0, pts, np.zeros(64, F32)), torch.Tensor) and "report" not in eng.kw
    opt = optimizer(None, True)
    opt.decoder = type("D", (), {"engine": eng})()
    got = opt.estimate_pose_cam_obj(np.eye(4, dtype=F32), 1.0, pts, np.zeros(64, F32))
    assert eng.kw["report"] is True and sorted(got.keys()) == ["observations", "t_cam_obj"] and got.observations["pt_alive"].all()


def test_tool_flag():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import reoptimise_map as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    p = inspect.signature(tool.reoptimise).parameters
    assert "report" in p and p["report"].default is False
    src = open(os.path.join(ROOT, "tools", "reoptimise_map.py")).read()
    assert '"--report"' in src and "FILE.npz" in src
