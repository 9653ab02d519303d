"""CPU: the host side of the posterior (include/dsp_gn.h dsp_batch_posterior, include/dsp_pose_graph.h dsp_pg_edge_information):
the edge's error coordinates, the host arithmetic, the condition of the recorded fixture systems, the elimination the device kernel runs
(restated in numpy, tests/posterior_ref.py) against a refined inverse, and the Python surface."""
import copy
import json
import os
import sys

import numpy as np
import pytest
from scipy.linalg import expm

import posterior_ref as R
from conftest import ROOT, golden
from dsp_slam_amd import _lib as L, pose_graph as P

PKG = os.path.join(ROOT, "dsp_slam_amd")
JOINT = ["golden_recon_small.npz", "golden_recon_cfg1.npz", "golden_recon_redwood.npz", "golden_recon_freiburg.npz", "golden_recon_cfg2.npz",
         "golden_recon_chairs32.npz", "golden_recon_cfg5.npz", "golden_recon_mono_shape.npz", "golden_recon_mono_wide.npz", "golden_recon_complex.npz",
         "golden_multiview_cars3.npz"]
# every golden_recon_*.npz but golden_recon_fail.npz: that run fails in its first iteration (fewer than 10 in-sphere samples), so the
# reference recorded no system for it (no it_H); test_every_recorded_system_is_listed keeps the list complete


def _random_rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _spd(rng, n, cond=1e4):
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    a = (q * np.geomspace(1.0, cond, n)) @ q.T
    return 0.5 * (a + a.T)


def _hat_sim3(d):
    v, w, s = d[:3], d[3:6], d[6]
    m = np.zeros((4, 4))
    m[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + s * np.eye(3)
    m[:3, 3] = v
    return m


def _rigid_of_inverse(t_oc):
    """T_co = T_oc^-1 = [s R | t] -> (the SE3Quat of [R | t], s)."""
    t_co = np.linalg.inv(t_oc)
    s = np.cbrt(np.linalg.det(t_co[:3, :3]))
    m = np.eye(4)
    m[:3, :3] = t_co[:3, :3] / s
    m[:3, 3] = t_co[:3, 3]
    return P.from_matrix(m), s


def test_edge_coordinates():
    """T_oc <- exp(delta) T_oc moves the edge error by [omega, upsilon] = [delta_w, s delta_v] (second order in delta: O(1e-4) relative)."""
    rng = np.random.default_rng(7)
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    worst_e, worst_q = 0.0, 0.0
    for _ in range(32):
        s = rng.uniform(0.5, 3.0)
        t_co = np.eye(4)
        t_co[:3, :3] = s * _random_rotation(rng)
        t_co[:3, 3] = rng.uniform(-5, 5, 3)
        t_oc = np.linalg.inv(t_co)
        delta = rng.normal(size=7)
        delta *= 1e-4 / np.linalg.norm(delta)
        meas, s0 = _rigid_of_inverse(t_oc)
        meas1, _ = _rigid_of_inverse(expm(_hat_sim3(delta)) @ t_oc)
        assert abs(s0 - s) < 1e-12 * s
        err = P.edge_error(meas, ident, meas1)                  # log(meas'^-1 * meas)
        want = np.concatenate([delta[3:6], s * delta[:3]])
        worst_e = max(worst_e, float(np.linalg.norm(err - want) / np.linalg.norm(err)))
        assert np.linalg.norm(err - want) <= 1e-3 * np.linalg.norm(err)
        s7 = _spd(rng, 7)
        omega = P.edge_information(s7, s)
        d = delta[:6]
        q_want = float(d @ R.marginalise_sigma(s7) @ d)
        q_got = float(err @ omega @ err)
        assert np.array_equal(omega, omega.T)                   # a symmetric input gives a bit-symmetric information matrix
        worst_q = max(worst_q, abs(q_got - q_want) / q_want)
        assert abs(q_got - q_want) <= 1e-3 * q_want
        chi2, _, _ = P.edge_chi2_info(err, omega)
        assert abs(chi2 - q_got) <= 1e-12 * q_got
    print("edge coordinates: worst relative deviation of err %.2e, of the quadratic form %.2e" % (worst_e, worst_q))


def test_host_arithmetic():
    rng = np.random.default_rng(11)
    lib = L.load()
    for dof in (6, 7):
        s = np.stack([_spd(rng, dof) for _ in range(16)])
        sc = rng.uniform(0.5, 3.0, 16)
        for gain in (1.0, 0.37):
            got = P.edge_information(s, sc, gain)
            assert got.shape == (16, 6, 6)
            for i in range(16):
                want = R.edge_information(s[i], sc[i], gain)
                assert np.abs(got[i] - want).max() <= 1e-12 * np.abs(want).max()
                assert np.all(np.linalg.eigvalsh(0.5 * (got[i] + got[i].T)) > 0)
        assert np.array_equal(P.edge_information(s[0], sc[0]), P.edge_information(s, sc)[0])
    err = rng.normal(size=(64, 6)) * np.geomspace(1e-3, 3.0, 64)[:, None]
    for c in (1e3, 2.5):
        for delta in (0.0, P.TH_HUBER_OBJECT_LOCAL_BA, 0.5):
            a = P.edge_chi2(err, c, delta)
            b = P.edge_chi2_info(err, np.broadcast_to(c * np.eye(6), (64, 6, 6)), delta)
            for x, y in zip(a, b):
                assert np.all(np.abs(x - y) <= 1e-14 * np.abs(x))
            if delta > 0 and c == 1e3:
                assert (a[2] < 1).any() and (a[2] == 1).any()       # both branches of the kernel
    # refused arguments
    out = np.zeros(36)
    ok7, one = np.ascontiguousarray(_spd(rng, 7)), np.ones(1)
    f = lib.dsp_pg_edge_information
    p = lambda a: L.ptr(a, L.c_f64p)
    assert f(1, 7, p(ok7), p(one), 1.0, p(out)) == 0
    assert f(1, 5, p(ok7), p(one), 1.0, p(out)) == -1 and f(1, 8, p(ok7), p(one), 1.0, p(out)) == -1
    assert f(1, 7, p(ok7), p(np.zeros(1)), 1.0, p(out)) == -1 and f(1, 7, p(ok7), p(-one), 1.0, p(out)) == -1
    assert f(1, 7, p(ok7), p(np.full(1, np.nan)), 1.0, p(out)) == -1
    bad = ok7.copy()
    bad[6, 6] = 0.0
    assert f(1, 7, p(bad), p(one), 1.0, p(out)) == -1
    assert f(1, 6, p(np.ascontiguousarray(bad[:6, :6])), p(one), 1.0, p(out)) == 0      # no sigma to marginalise
    assert f(1, 7, None, p(one), 1.0, p(out)) == -1 and f(1, 7, p(ok7), p(one), 1.0, None) == -1 and f(-1, 7, p(ok7), p(one), 1.0, p(out)) == -1
    assert f(0, 7, None, None, 1.0, None) == 0
    g = lib.dsp_pg_edge_chi2_info
    e6, o66, c1 = np.ones(6), np.ascontiguousarray(np.eye(6)), np.zeros(1)
    assert g(1, p(e6), p(o66), 0.0, p(c1), None, None) == 0 and c1[0] == 6.0
    assert g(1, p(e6), None, 0.0, p(c1), None, None) == -1 and g(1, None, p(o66), 0.0, p(c1), None, None) == -1
    with pytest.raises(ValueError):
        P.edge_information(np.eye(5), 1.0)


def _undamped_reference_systems(name):
    """[(Lambda (n, n) float64, n_pose)] of every recorded state: the reference's it_H minus its damping."""
    g = golden(name)
    h = g["it_H"].astype(np.float64)
    if h.shape[-1] == 6:
        return [(h[e] - 1e-2 * np.eye(6), 6) for e in range(h.shape[0])]
    s_damp = float(np.float32(json.loads(str(g["cfg_json"]))["optimizer"]["joint_optim"]["scale_damping"]))
    damp = np.zeros(h.shape[-1])
    damp[:7] = 1.0
    damp[6] += s_damp
    return [(h[e] - np.diag(damp), 7) for e in range(h.shape[0])]


def test_every_recorded_system_is_listed():
    have = sorted(f for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.startswith("golden_recon_") and f.endswith(".npz"))
    assert sorted(JOINT[:-1] + ["golden_recon_fail.npz"]) == have
    assert "it_H" not in golden("golden_recon_fail.npz").files


@pytest.mark.parametrize("name", JOINT + ["golden_pose_only_8it.npz"])
def test_fixture_condition(name):
    """The singularity rule is a stated condition (a pivot <= 16 FLT_EPSILON x its own diagonal entry is round-off of the fp32 Gram
    chains).  No recorded state of any fixture comes near it, in either elimination order -- noticed HERE if a fixture ever does."""
    worst, cond = np.inf, 0.0
    for lam, n_pose in _undamped_reference_systems(name):
        assert np.all(np.linalg.eigvalsh(0.5 * (lam + lam.T)) > 0)
        r = R.pivot_ratios(0.5 * (lam + lam.T), n_pose)
        worst, cond = min(worst, *r), max(cond, float(np.linalg.cond(lam)))
    print(name, "smallest pivot / diagonal %.3g, largest condition number %.3g" % (worst, cond))
    assert worst > 100 * R.SINGULAR_RATIO


@pytest.mark.parametrize("name", ["golden_recon_small.npz", "golden_recon_freiburg.npz", "golden_recon_chairs32.npz", "golden_multiview_cars3.npz",
                                  "golden_pose_only_8it.npz"])
def test_elimination_against_refined_inverse(name):
    """The kernel's elimination (restated: posterior_ref.sweep) on the undamped reference systems: each output within
    max(8 e_lapack, 1e-13) of the refined inverse, like the device's in tests/test_gpu_posterior.py."""
    lam, n_pose = _undamped_reference_systems(name)[-1]
    lam = 0.5 * (lam + lam.T)
    got = R.sweep(lam, n_pose)
    assert got["status"] == 0
    ref = R.marginals(R.refined_inverse(lam), n_pose)
    lap = R.marginals(np.linalg.inv(lam), n_pose)
    for key, r, l in zip(("cov_pose", "var_code", "info_pose"), ref, lap):
        if r.size == 0:
            continue
        e_dev, e_lap = R.rel_err(got[key], r), R.rel_err(l, r)
        print(name, key, "error %.2e, lapack %.2e, ratio %.2f" % (e_dev, e_lap, e_dev / max(e_lap, 1e-300)))
        assert e_dev <= max(8 * e_lap, 1e-13)
        assert np.array_equal(got[key], got[key].T) or got[key].ndim == 1
    assert np.all(got["var_code"] > 0)
    # a rank-deficient system is flagged, not inverted
    j = np.random.default_rng(3).normal(size=(3, 6))
    assert R.sweep(j.T @ j, 6)["status"] == 2


@pytest.fixture()
def mirror():
    sys.path.insert(0, PKG)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    yield
    sys.path.remove(PKG)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]


def test_python_surface(mirror):
    from reconstruct.utils import ForceKeyErrorDict
    from reconstruct.optimizer import Optimizer
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    base.setdefault("data_type", "KITTI")
    opt = Optimizer(None, ForceKeyErrorDict(copy.deepcopy(base)))
    assert opt.posterior_joint is None and opt.posterior_pose_only is None
    for wj, wp in (("sum", None), (None, "mean"), ("mean", "sum")):
        cfg = copy.deepcopy(base)
        if wj:
            cfg["optimizer"]["joint_optim"]["posterior"] = wj
        if wp:
            cfg["optimizer"]["pose_only_optim"]["posterior"] = wp
        opt = Optimizer(None, ForceKeyErrorDict(cfg))
        assert opt.posterior_joint == wj and opt.posterior_pose_only == wp
        assert opt.convergence_joint is None and opt.convergence_pose_only is None          # the other additions stay off
    cfg = copy.deepcopy(base)
    cfg["optimizer"]["joint_optim"]["posterior"] = "median"
    with pytest.raises(ValueError):
        Optimizer(None, ForceKeyErrorDict(cfg))
    # the ABI: the new names are exported, bound, and outside the dsp_batch_set_ family
    lib = L.load()
    for n in ("dsp_batch_posterior", "dsp_batch_posterior_fetch", "dsp_pg_edge_information", "dsp_pg_edge_chi2_info"):
        assert hasattr(lib, n)
    assert (L.POSTERIOR_MEAN, L.POSTERIOR_SUM, L.POSTERIOR_OK, L.POSTERIOR_NONE, L.POSTERIOR_SINGULAR) == (0, 1, 0, 1, 2)
    from dsp_slam_amd import engine as E
    assert E._posterior_args("sum") == (1, "sum") and E._posterior_args((2, "mean")) == (2, "mean")
    assert E._posterior_weights("sum") == 1 and E._posterior_weights("mean") == 0
    with pytest.raises(ValueError):
        E._posterior_weights("both")
