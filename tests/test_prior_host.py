"""CPU: the Gaussian prior on pose and code (include/dsp_gn.h: dsp_batch_prior) -- the Lie-group maths restated in numpy
(tests/prior_ref.py), the finite-difference arbiter of the jacobian's signs, the arithmetic the device kernel runs (csrc/prior_math.h,
compiled for the host behind dsp_debug_prior_terms) against that restatement, the argument checks, and the Python / tool plumbing."""
import ctypes as C
import importlib.util
import inspect
import os
import sys

import numpy as np
import pytest

import prior_ref as R
from conftest import ROOT
from dsp_slam_amd import _lib as L

PKG = os.path.join(ROOT, "dsp_slam_amd")


def _unit(rng, n):
    x = rng.normal(size=n)
    return x / np.linalg.norm(x)


def _xi(rng, theta, sigma, vmax=3.0, dof=7):
    xi = np.concatenate([rng.uniform(-vmax, vmax, 3), theta * _unit(rng, 3), [sigma]])
    return xi[:dof]


def test_exp_log_round_trip():
    """Exp(Log(T)) == T to 1e-12 for random Sim(3) and SE(3) elements with rotation angles up to 3 rad."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(64):
        xi = _xi(rng, rng.uniform(0.0, 3.0), rng.uniform(-1.5, 1.5) if k % 2 else 0.0)
        t = R.Exp(xi)
        e = R.Log(t)
        worst = max(worst, np.abs(R.Exp(e) - t).max() / max(1.0, np.abs(t).max()), np.abs(e - xi).max() / max(1.0, np.abs(xi).max()))
        if k % 2 == 0:
            assert abs(e[6]) < 1e-14                       # SE(3): sigma is 0 up to round-off
    print("worst round-trip error %.2e" % worst)
    assert worst < 1e-12


@pytest.mark.parametrize("theta,sigma", [(0.0, 0.0), (1e-9, 0.0), (0.0, 1e-9), (1e-9, 1e-9), (0.0, 0.7), (1.3, 0.0), (1e-9, -0.7), (2.0, 1e-9)])
def test_round_trip_at_the_series_branches(theta, sigma):
    rng = np.random.default_rng(5)
    xi = _xi(rng, theta, sigma)
    t = R.Exp(xi)
    e = R.Log(t)
    assert np.abs(R.Exp(e) - t).max() < 1e-12
    assert np.abs(e - xi).max() < 1e-12


def _lib_terms(t_oc, z, t0, z0, lam, pose_only=False, code_len=64):
    """One object's prior terms by the arithmetic the device runs, on the host: (rc, extra n x (n + 1), e, chi2)."""
    n, P = (6, 6) if pose_only else (71, 7)
    extra, e, chi2 = np.zeros((n, n + 1)), np.zeros(P + 64), np.zeros(1)
    f = lambda a: None if a is None else L.f32(a)
    t_oc, t0, z, z0 = f(t_oc), f(t0), f(z), f(z0)
    lam = np.ascontiguousarray(lam, np.float64)
    rc = L.load().dsp_debug_prior_terms(int(pose_only), code_len, L.ptr(t_oc), L.ptr(z), L.ptr(t0), L.ptr(z0), L.ptr(lam, L.c_f64p),
                                        L.ptr(extra, L.c_f64p), L.ptr(e, L.c_f64p), L.ptr(chi2, L.c_f64p))
    return rc, extra, e, float(chi2[0])


@pytest.mark.parametrize("theta,sigma", [(0.0, 0.0), (1e-9, 1e-9), (1e-5, 0.3), (0.1, 0.0), (0.2499, -0.9), (0.2, 1.2), (0.24, -2.5), (0.25, 0.4),
                                         (1.0, 1e-9), (2.0, -0.5), (3.0, 0.8), (3.1, 0.0)])
def test_library_log_matches_the_restatement(theta, sigma):
    """The library's logarithm (closed forms for theta >= 1/4, series below; moments by the backward recurrence for |sigma| < 1, the forward one
    otherwise) against the Taylor-series restatement, on the SAME float32 matrices: 1e-11 of the residual's size.  (The float32 matrices are
    not exact Sim(3) elements, so this compares two evaluations of one definition, not a round trip.)"""
    rng = np.random.default_rng(int(1000 * theta) + 17)
    lam = np.eye(71)
    for _ in range(4):
        t0 = R.Exp(_xi(rng, rng.uniform(0, 3), rng.uniform(-0.5, 0.5))).astype(np.float32)
        t_oc = (R.Exp(_xi(rng, theta, sigma, vmax=1.0)) @ t0.astype(np.float64)).astype(np.float32)
        z, z0 = rng.normal(size=64).astype(np.float32), rng.normal(size=64).astype(np.float32)
        ref = R.terms(t_oc, z, t0, z0, lam)
        rc, _, e, chi2 = _lib_terms(t_oc, z, t0, z0, lam)
        assert rc == 0 and ref is not None
        assert np.abs(e - ref["e"]).max() <= 1e-11 * max(1.0, np.abs(ref["e"]).max())
        assert abs(chi2 - ref["chi2"]) <= 1e-11 * ref["chi2"]


def test_bch_jacobian_by_finite_differences():
    """The arbiter of the jacobian's signs: (Log(Exp(d) Exp(e)) - Log(Exp(-d) Exp(e))) / 2 against J_p(e) d with |d| = 1e-6 (the central
    difference of Log(Exp(d) Exp(e)) - e: its error is third order in d), for |e| in {0, 0.1, 0.5}.

    J_p keeps the BCH series of the inverse left jacobian up to ad^2 / 12; the first term left out is -ad^4 / 720, so the relative residual
    must stay below ||ad(e)||^4 / 720 (plus 2 % for the ad^6 / 30240 term and 1e-8 for the differences' round-off) and must shrink as the
    fourth power of |e|.  A wrong sign in J_p or ad leaves a residual of first or second order in |e| instead (0.05 ... 0.25 at |e| = 0.5).
    Observed (8 directions each): |e| = 0: 2.6e-11 ... 1.1e-10; |e| = 0.1: 1.6e-8 ... 7.1e-8; |e| = 0.5: 1.0e-5 ... 4.5e-5, i.e. 0.10 ... 0.46
    of the bound; ratio of the two 625 ... 629 against 5^4 = 625."""
    rng = np.random.default_rng(23)
    for _ in range(8):
        eu, d = _unit(rng, 7), 1e-6 * _unit(rng, 7)
        res = {}
        for mag in (0.0, 0.1, 0.5):
            e = mag * eu
            te = R.Exp(e)
            fd = 0.5 * (R.Log(R.Exp(d) @ te) - R.Log(R.Exp(-d) @ te))
            res[mag] = np.linalg.norm(fd - R.jac_pose(e) @ d) / np.linalg.norm(d)
            a4 = np.linalg.norm(R.ad(e), 2) ** 4
            print("|e| = %.1f: residual %.3e, bound %.3e" % (mag, res[mag], a4 / 720.0))
            assert res[mag] <= 1.02 * a4 / 720.0 + 1e-8
        assert 0.5 * 625 < res[0.5] / res[0.1] < 2.0 * 625
    # pose-only: the top-left 6 x 6 with sigma = 0 is the SE(3) jacobian
    e6, d6 = 0.3 * _unit(rng, 6), 1e-6 * _unit(rng, 6)
    te = R.Exp(e6)
    fd = 0.5 * (R.Log(R.Exp(d6) @ te) - R.Log(R.Exp(-d6) @ te))[:6]
    assert np.linalg.norm(fd - R.jac_pose(np.concatenate([e6, [0.0]]), 6) @ d6) / 1e-6 <= 1.02 * np.linalg.norm(R.ad(np.concatenate([e6, [0.0]])), 2) ** 4 / 720 + 1e-8


def _spd(rng, n, scale=1.0):
    a = rng.normal(size=(n, n))
    m = a @ a.T * scale
    return np.ascontiguousarray(0.5 * (m + m.T))


@pytest.mark.parametrize("pose_only,code_len", [(False, 64), (False, 32), (True, 64)])
def test_library_terms_match_the_restatement(pose_only, code_len):
    """[J^T Lp J | -J^T Lp e] of the library against numpy: 1e-12 of each block's largest entry (fp64 sums of at most 71 terms)."""
    rng = np.random.default_rng(3 + code_len + pose_only)
    n = 6 if pose_only else 71
    live = n if pose_only else 7 + code_len
    lam = np.zeros((n, n))
    lam[:live, :live] = _spd(rng, live, 10.0)
    t0 = R.Exp(_xi(rng, 1.0, 0.2)).astype(np.float32)
    t_oc = (R.Exp(_xi(rng, 0.4, 0.0 if pose_only else 0.1, vmax=0.3)) @ t0.astype(np.float64)).astype(np.float32)
    z, z0 = rng.normal(size=64).astype(np.float32), rng.normal(size=64).astype(np.float32)
    ref = R.terms(t_oc, z, t0, z0, lam, pose_only, code_len)
    rc, extra, e, chi2 = _lib_terms(t_oc, None if pose_only else z, t0, None if pose_only else z0, lam, pose_only, code_len)
    assert rc == 0
    H, b = extra[:, :n], extra[:, n]
    assert np.array_equal(H, H.T)                                   # symmetric bit for bit: the solve is pivot-free
    assert np.abs(H - ref["H"]).max() <= 1e-12 * np.abs(ref["H"]).max()
    assert np.abs(b - ref["b"]).max() <= 1e-12 * np.abs(ref["b"]).max()
    assert np.all(H[live:] == 0) and np.all(H[:, live:] == 0) and np.all(b[live:] == 0)
    assert np.abs(e[:ref["e"].shape[0]] - ref["e"]).max() <= 1e-12 * np.abs(ref["e"]).max()
    assert abs(chi2 - ref["chi2"]) <= 1e-12 * ref["chi2"]
    if pose_only:
        assert np.all(e[6:] == 0)


def test_half_a_turn_is_refused():
    rot_y = np.diag([-1.0, 1.0, -1.0, 1.0])
    t0 = R.Exp(np.array([0.1, -0.2, 2.0, 0.3, 0.1, -0.2, 0.1])).astype(np.float32)
    t_oc = (rot_y @ t0.astype(np.float64)).astype(np.float32)
    z = np.zeros(64, np.float32)
    assert R.terms(t_oc, z, t0, z, np.eye(71)) is None
    assert _lib_terms(t_oc, z, t0, z, np.eye(71))[0] == -4          # DSP_E_STATE: where the device ends the object DSP_OBJ_NAN
    just_inside = (R.Exp(np.array([0, 0, 0, 0, np.pi - 2e-3, 0, 0])) @ t0.astype(np.float64))
    assert R.terms(just_inside, z, t0, z, np.eye(71)) is not None


def _check(pose_only, code_len, t0, z0, lam):
    f = lambda a: None if a is None else L.f32(a)
    t0, z0 = f(t0), f(z0)
    lam = None if lam is None else np.ascontiguousarray(lam, np.float64)
    n = 0 if lam is None else lam.shape[0]
    return L.load().dsp_debug_prior_check(int(pose_only), code_len, n, L.ptr(t0), L.ptr(z0), L.ptr(lam, L.c_f64p))


def test_argument_checks():
    """dsp_batch_prior's host-side checks (the same function, reached without a batch): each one refuses with DSP_E_ARG."""
    rng = np.random.default_rng(2)
    E_ARG = -1
    t0 = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    z0 = np.zeros((2, 64), np.float32)
    lam = np.stack([_spd(rng, 71), np.zeros((71, 71))])
    assert _check(False, 64, t0, z0, lam) == 0
    assert _check(True, 64, t0, None, np.stack([_spd(rng, 6)] * 2)) == 0                    # pose-only: code0 is ignored
    assert _check(False, 64, t0, None, lam) == E_ARG and _check(False, 64, None, z0, lam) == E_ARG       # some, not all, given

    def broken(edit, code_len=64):
        t, z, l = t0.copy(), z0.copy(), lam.copy()
        edit(t, z, l)
        return _check(False, code_len, t, z, l)
    assert broken(lambda t, z, l: l.__setitem__((0, 3, 4), np.nan)) == E_ARG                  # non-finite input
    assert broken(lambda t, z, l: t.__setitem__((0, 0, 3), np.inf)) == E_ARG
    assert broken(lambda t, z, l: z.__setitem__((0, 5), np.nan)) == E_ARG
    assert broken(lambda t, z, l: t.__setitem__((0, 0, 0), -1.0)) == E_ARG                    # det(T0[:3, :3]) <= 0
    assert broken(lambda t, z, l: t.__setitem__((0, 2), 0.0)) == E_ARG
    assert broken(lambda t, z, l: l.__setitem__((0, 3, 4), np.nextafter(l[0, 4, 3], np.inf))) == E_ARG      # not symmetric bit for bit
    assert broken(lambda t, z, l: l.__setitem__((0, 9, 9), -1e-300)) == E_ARG                 # a negative diagonal entry
    assert broken(lambda t, z, l: None, code_len=32) == E_ARG                                 # non-zero beyond a 32-D decoder's code length
    l32 = lam.copy()
    l32[:, 39:, :] = 0.0
    l32[:, :, 39:] = 0.0
    assert _check(False, 32, t0, z0, l32) == 0
    # an object without a prior (Lambda all zero): its t0 and code0 are not looked at
    assert broken(lambda t, z, l: (t.__setitem__(1, 0.0), z.__setitem__(1, np.nan))) == 0
    # a stale token, without a device
    lib = L.load()
    assert lib.dsp_batch_prior(C.c_void_p(0x1234), None, None, None) == E_ARG
    assert lib.dsp_batch_prior_fetch(C.c_void_p(0x1234), None, None) == E_ARG


@pytest.fixture()
def mirror():
    sys.path.insert(0, PKG)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    yield
    sys.path.remove(PKG)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]


class _FakeEngine(object):
    """Records what the Optimizer hands down; returns results shaped like the Engine's."""

    def __init__(self):
        self.calls = []

    def reconstruct_batch(self, prm, t, pts, rays, depth, codes=None, **kw):
        self.calls.append(("joint", kw))
        n = len(pts)
        res = (np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), np.zeros((n, 64), np.float32), np.ones(n, np.float32), np.zeros(n, np.int32))
        return res + ((dict(e=np.arange(n * 71.0).reshape(n, 71), chi2=np.arange(n) + 2.5),) if "prior" in kw else ())

    def estimate_pose_batch(self, prm, t, scale, pts, codes, **kw):
        self.calls.append(("pose", kw))
        out = np.tile(np.eye(4, dtype=np.float32), (len(pts), 1, 1))
        return (out, dict(e=np.ones((len(pts), 6)), chi2=np.full(len(pts), 7.0))) if "prior" in kw else out


def test_python_and_tool_plumbing(mirror):
    import copy
    import json
    from reconstruct.utils import ForceKeyErrorDict
    from reconstruct.optimizer import Optimizer
    from dsp_slam_amd import engine as E
    lib = L.load()
    names = [s[0] for s in L.SYMBOLS]
    for n in ("dsp_batch_prior", "dsp_batch_prior_fetch", "dsp_debug_prior_check", "dsp_debug_prior_terms"):
        assert hasattr(lib, n) and n in names and not n.startswith("dsp_batch_set_")
    # new keyword arguments only, default None
    for fn, kw in ((E.Engine.reconstruct_batch, "prior"), (E.Engine.reconstruct_multiview_batch, "prior"), (E.Engine.estimate_pose_batch, "prior"),
                   (Optimizer.reconstruct_object, "prior"), (Optimizer.estimate_pose_cam_obj, "prior"), (Optimizer.reconstruct_object_multiview, "prior")):
        p = inspect.signature(fn).parameters[kw]
        assert p.default is None and list(inspect.signature(fn).parameters)[-1] == kw
    assert hasattr(E.Batch, "set_prior") and hasattr(E.Batch, "prior_residual")
    rec = dict(t_obj_cam=np.eye(4), code=np.ones(64), Lambda=np.eye(71))
    assert E._prior_args(rec)[2] is rec["Lambda"] and E._prior_args((1, 2, 3)) == (1, 2, 3)
    # the Optimizer: one posterior row goes down as per-object arrays; objects without a prior get Lambda = 0
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    base.setdefault("data_type", "KITTI")
    opt = Optimizer(None, ForceKeyErrorDict(copy.deepcopy(base)))
    opt.verbose = False
    eng = _FakeEngine()
    opt.decoder = type("D", (), {"engine": eng})()
    pts, rays, depth = np.zeros((4, 3), np.float32), np.zeros((6, 3), np.float32), np.zeros(4, np.float32)
    plain = opt.reconstruct_object(np.eye(4), pts, rays, depth)
    assert "prior" not in eng.calls[-1][1] and sorted(plain.keys()) == ["code", "is_good", "loss", "t_cam_obj"]
    got = opt.reconstruct_object(np.eye(4), pts, rays, depth, prior=rec)
    kw = eng.calls[-1][1]["prior"]
    assert kw["Lambda"].shape == (1, 71, 71) and kw["Lambda"].dtype == np.float64 and np.array_equal(kw["Lambda"][0], np.eye(71))
    assert kw["t_obj_cam"].shape == (1, 4, 4) and kw["code"].shape == (1, 64) and np.all(kw["code"] == 1)
    assert got.prior_chi2 == 2.5 and got.prior_residual.shape == (71,)
    both = opt.reconstruct_objects([np.eye(4)] * 2, [pts] * 2, [rays] * 2, [depth] * 2, priors=[None, rec])
    kw = eng.calls[-1][1]["prior"]
    assert not kw["Lambda"][0].any() and kw["Lambda"][1].any() and both[1].prior_chi2 == 3.5
    pose = opt.estimate_pose_cam_obj(np.eye(4), 1.0, pts, np.zeros(64))
    assert "prior" not in eng.calls[-1][1] and tuple(pose.shape) == (4, 4)
    pose = opt.estimate_pose_cam_obj(np.eye(4), 1.0, pts, np.zeros(64), prior=dict(t_obj_cam=np.eye(4), Lambda=2 * np.eye(6)))
    assert eng.calls[-1][1]["prior"]["Lambda"].shape == (1, 6, 6) and pose.prior_chi2 == 7.0 and pose.prior_residual.shape == (6,)
    # the tool: records matched by id, skipped when not ok, re-based to the observing camera
    spec = importlib.util.spec_from_file_location("reoptimise_map", os.path.join(ROOT, "tools", "reoptimise_map.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert {"prior", "posterior_level"} <= set(inspect.signature(tool.reoptimise).parameters)
    src = open(os.path.join(ROOT, "tools", "reoptimise_map.py")).read()
    assert '"--prior"' in src and '"--posterior-level"' in src
    cam_old, cam_new = R.Exp(np.array([1, 2, 3, 0.1, 0.2, 0.3])), R.Exp(np.array([-1, 0, 2, 0.3, -0.2, 0.1]))
    t_oc_old = R.Exp(np.array([0.5, 0.1, -2.0, 0.2, 0.1, 0.0, 0.3]))
    prior = dict(ids=np.array([7, 9, 4]), status=np.array([0, 2, 0]), t_obj_cam=np.stack([t_oc_old] * 3), code=np.ones((3, 64), np.float32),
                 Lambda=np.stack([np.eye(71)] * 3), t_world_cam=np.stack([cam_old] * 3))
    objs = [dict(id=4), dict(id=5), dict(id=9), dict(id=7)]
    obs = [dict(t_world_cam=cam_old), None, dict(t_world_cam=cam_new), dict(t_world_cam=cam_new)]
    t0, z0, lam = tool.prior_arrays(prior, objs, obs, [0, 2, 3])
    assert lam[0].any() and not lam[1].any() and lam[2].any()                # id 9's record is singular: no prior
    assert np.abs(t0[0] - t_oc_old).max() < 1e-6                              # same camera: unchanged
    # T_oc maps camera points to the object: the re-based prior maps the SAME world point to the same object point
    x_world = np.array([0.3, -0.2, 5.0, 1.0])
    assert np.abs(t0[2].astype(np.float64) @ np.linalg.inv(cam_new) @ x_world - t_oc_old @ np.linalg.inv(cam_old) @ x_world).max() < 1e-5
