"""CPU tier of the mask of unknowns (dsp_batch_unknowns, include/dsp_gn.h): bindings, argument checks, the named groups, keyword and
config plumbing, the conditioned fp64 reference (tests/unknowns_ref.py) that tests/test_gpu_unknowns.py holds the device to, and the
exactness argument of the solve step -- a pinned row gives dx_i == 0.0 and leaves the live block the arithmetic of the reduced system --
checked on the emulations of its elimination schedules."""
import copy
import ctypes as C
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

import posterior_ref as R
import solve_emulator as S
import unknowns_ref as U
from conftest import ROOT
from dsp_slam_amd import _lib as L, engine as E
from test_gn_metric import _state
from test_solve_schedule import LDA, NS1, per_panel

F32 = np.float32
U8P = C.POINTER(C.c_uint8)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_bindings_and_header():
    bound = {n: (r, a) for n, r, a in L.SYMBOLS}
    assert bound["dsp_batch_unknowns"][0] is C.c_int and bound["dsp_batch_unknowns"][1][0] is C.c_void_p and len(bound["dsp_batch_unknowns"][1]) == 2
    assert bound["dsp_debug_unknowns_check"][0] is C.c_int and bound["dsp_debug_unknowns_check"][1][:3] == [C.c_int, C.c_int, C.c_int]
    hdr = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    assert re.search(r"int dsp_batch_unknowns\(dsp_batch\* b, const uint8_t\* live\);", hdr)
    assert re.search(r"int dsp_debug_unknowns_check\(int pose_only, int code_len, int n_objects, const uint8_t\* live\);", hdr)
    assert not re.search(r"dsp_batch_set_\w*unknown", hdr)
    lib = L.load()
    assert hasattr(lib, "dsp_batch_unknowns") and hasattr(lib, "dsp_debug_unknowns_check")
    assert lib.dsp_abi_version() == L.ABI_VERSION == 6
    assert lib.dsp_batch_unknowns(None, None) == -1                                # a stale token: DSP_E_ARG
    ones = np.ones(71, np.uint8)
    assert lib.dsp_batch_unknowns(None, L.ptr(ones, U8P)) == -1
    assert callable(E.Batch.set_unknowns) and E.MultiviewBatch.set_unknowns is E.Batch.set_unknowns


def _check(live, pose_only=0, code_len=64, n=None):
    m = None if live is None else np.ascontiguousarray(live, np.uint8)
    w = 6 if pose_only else 71
    n = (0 if m is None else m.size // w) if n is None else n
    return L.load().dsp_debug_unknowns_check(pose_only, code_len, n, L.ptr(m, U8P))


def test_argument_checks():
    rng = np.random.default_rng(1)
    assert _check(np.ones((3, 71))) == 0 and _check(np.zeros((3, 71))) == 0 and _check(rng.integers(0, 2, (5, 71))) == 0
    assert _check(None, n=4) == 0                                                  # NULL = all live: nothing to check
    assert _check(np.ones((2, 6)), pose_only=1) == 0 and _check(np.zeros((2, 6)), pose_only=1) == 0 and _check(rng.integers(0, 2, (4, 6)), pose_only=1) == 0
    for pos in (0, 6, 7, 70):
        m = np.ones((2, 71), np.uint8)
        m[1, pos] = 2
        assert _check(m) == -1, pos
        m[1, pos] = 255
        assert _check(m) == -1, pos
    for pos in range(6):
        m = np.ones((2, 6), np.uint8)
        m[0, pos] = 2
        assert _check(m, pose_only=1) == -1
    # a 32-D decoder: slots at or beyond 7 + 32 are not looked at, the ones in front of them are
    m = np.ones((2, 71), np.uint8)
    m[:, 39:] = 2
    assert _check(m, code_len=32) == 0 and _check(m, code_len=64) == -1
    m[0, 38] = 2
    assert _check(m, code_len=32) == -1
    assert _check(None, n=-1) == -1 and _check(np.ones((1, 71)), code_len=48) == -1


# ---- the named groups ------------------------------------------------------------------------------------------------------------------
def test_unknowns_mask_group_arithmetic():
    m = E.unknowns_mask
    assert m("all").tolist() == [1] * 71 and m([]).tolist() == [0] * 71 and m("all").dtype == np.uint8
    assert np.nonzero(m(["translation"]))[0].tolist() == [0, 1, 2] and np.nonzero(m(["rotation"]))[0].tolist() == [3, 4, 5]
    assert np.nonzero(m(["yaw"]))[0].tolist() == [4] and np.nonzero(m(["scale"]))[0].tolist() == [6]
    assert np.nonzero(m(["pose"]))[0].tolist() == list(range(7)) and np.nonzero(m(["code"]))[0].tolist() == list(range(7, 71))
    assert np.array_equal(m(["pose", "code"]), m("all")) and np.array_equal(m(["translation", "rotation", "scale"]), m("pose"))
    assert np.array_equal(m(["translation", "rotation", "code"]), 1 - m("scale"))             # known scale
    assert np.nonzero(m(["translation", "yaw", "scale", "code"]) == 0)[0].tolist() == [3, 5]   # the hard upright constraint
    assert np.array_equal(m(["yaw", "rotation"]), m("rotation")) and np.array_equal(m(["code", "code"]), m("code"))
    # pose-only batches: six SE(3) entries; scale and code name nothing there
    assert m("all", True).tolist() == [1] * 6 and m("pose", True).tolist() == [1] * 6 and m(["scale", "code"], True).tolist() == [0] * 6
    assert m(["translation", "yaw"], True).tolist() == [1, 1, 1, 0, 1, 0]
    for bad in ("poses", "", "Yaw", 3):
        with pytest.raises(ValueError):
            m([bad])
    assert _check(np.stack([m("pose"), m("code"), m([])])) == 0


# ---- Python plumbing -------------------------------------------------------------------------------------------------------------------
def test_engine_keyword_sits_in_front_of_obs_weights():
    for fn in (E.Engine.reconstruct_batch, E.Engine.reconstruct_multiview_batch, E.Engine.estimate_pose_batch):
        p = inspect.signature(fn).parameters
        assert list(p)[-4:] == ["unknowns", "obs_weights", "report", "prior"] and p["unknowns"].default is None
    assert list(inspect.signature(E.Batch.set_unknowns).parameters) == ["self", "live"] and inspect.signature(E.Batch.set_unknowns).parameters["live"].default is None


class _RecordingBatch(E.Batch):
    """Batch.set_unknowns without a device: the library call is recorded."""

    def __init__(self, n, pose_only=False):
        self.n, self.pose_only, self._h = n, pose_only, C.c_void_p()
        self.engine = type("Eng", (), {"_h": None})()


def test_set_unknowns_shapes(monkeypatch):
    seen = []

    class FakeLib(object):
        def dsp_batch_unknowns(self, h, p):
            seen.append(None if not p else np.ctypeslib.as_array(p, shape=(10000,)))
            return 0
    monkeypatch.setattr(L, "load", lambda: FakeLib())

    def sent(b, live):
        seen.clear()
        b.set_unknowns(live)
        w = 6 if b.pose_only else 71
        return None if seen[0] is None else seen[0][:b.n * w].reshape(b.n, w).copy()
    b = _RecordingBatch(3)
    assert sent(b, None) is None
    assert np.array_equal(sent(b, ["pose"]), np.tile(E.unknowns_mask("pose"), (3, 1)))
    assert np.array_equal(sent(b, "code"), np.tile(E.unknowns_mask("code"), (3, 1)))
    assert np.array_equal(sent(b, []), np.zeros((3, 71), np.uint8))
    per = sent(b, [["pose"], ["code"], []])
    assert np.array_equal(per, np.stack([E.unknowns_mask("pose"), E.unknowns_mask("code"), E.unknowns_mask([])]))
    row = np.random.default_rng(2).integers(0, 2, 71)
    assert np.array_equal(sent(b, row), np.tile(row, (3, 1)))                      # one row for every object
    full = np.random.default_rng(3).integers(0, 2, (3, 71))
    assert np.array_equal(sent(b, full), full) and np.array_equal(sent(b, full.astype(bool)), full)
    two = full.copy()
    two[1, 5] = 2
    assert sent(b, two)[1, 5] == 2                                                 # handed to the library, which refuses it
    for bad in (np.ones((2, 71)), np.ones(6), np.ones((3, 70))):
        with pytest.raises(ValueError):
            b.set_unknowns(bad)
    with pytest.raises(ValueError):
        b.set_unknowns(["pose", "shape"])
    p = _RecordingBatch(2, pose_only=True)
    assert np.array_equal(sent(p, ["translation", "yaw"]), np.tile([1, 1, 1, 0, 1, 0], (2, 1)))
    assert np.array_equal(sent(p, np.array([0, 0, 0, 1, 1, 1])), np.tile([0, 0, 0, 1, 1, 1], (2, 1)))
    with pytest.raises(ValueError):
        p.set_unknowns(np.ones((2, 71)))


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


class FakeEngine(object):
    def _four(self, n):
        return (np.tile(np.eye(4, dtype=F32), (n, 1, 1)), np.zeros((n, 64), F32), np.zeros(n, F32), np.zeros(n, np.int32))

    def reconstruct_batch(self, prm, t, pts, rays, depth, codes=None, **kw):
        self.kw = kw
        return self._four(len(pts))

    def reconstruct_multiview_batch(self, prm, t, views, codes=None, **kw):
        self.kw = kw
        return self._four(len(views))

    def estimate_pose_batch(self, prm, t, scale, pts, codes, **kw):
        self.kw = kw
        return np.tile(np.eye(4, dtype=F32), (len(pts), 1, 1))


def _config():
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    cfg.setdefault("data_type", "KITTI")
    return cfg


def test_optimizer_keyword_and_config(mirror):
    from reconstruct.optimizer import Optimizer
    from reconstruct.utils import ForceKeyErrorDict
    for fn in (Optimizer.reconstruct_object, Optimizer.reconstruct_object_multiview, Optimizer.estimate_pose_cam_obj):
        p = inspect.signature(fn).parameters
        assert list(p)[-3:] == ["unknowns", "obs_weights", "prior"] and p["unknowns"].default is None
    for fn in (Optimizer.reconstruct_objects, Optimizer.estimate_poses_cam_obj):
        p = inspect.signature(fn).parameters
        assert list(p)[-3:] == ["unknowns", "obs_weights", "priors"] and p["unknowns"].default is None

    def make(cfg):
        opt = Optimizer(None, ForceKeyErrorDict(cfg))
        opt.verbose = False
        eng = FakeEngine()
        opt.decoder = type("D", (), {"engine": eng})()
        return opt, eng
    pts, rays, depth = np.zeros((4, 3), F32), np.zeros((6, 3), F32), np.zeros(4, F32)
    eye = np.eye(4, dtype=F32)
    views = [dict(t_ref_cam=eye, pts=pts, rays=rays, depth=depth)]
    import torch
    # absent key -> no `unknowns` keyword passed, on any call
    opt, eng = make(_config())
    assert opt.unknowns_joint is None and opt.unknowns_pose_only is None
    plain = opt.reconstruct_object(eye, pts, rays, depth)
    assert "unknowns" not in eng.kw and sorted(plain.keys()) == ["code", "is_good", "loss", "t_cam_obj"]
    opt.reconstruct_objects([eye] * 2, [pts] * 2, [rays] * 2, [depth] * 2)
    assert "unknowns" not in eng.kw
    opt.reconstruct_object_multiview(eye, views)
    assert "unknowns" not in eng.kw
    assert isinstance(opt.estimate_pose_cam_obj(eye, 1.0, pts, np.zeros(64, F32)), torch.Tensor) and "unknowns" not in eng.kw
    # the call's keyword
    got = opt.reconstruct_object(eye, pts, rays, depth, unknowns=["pose"])
    assert eng.kw["unknowns"] == ["pose"] and sorted(got.keys()) == ["code", "is_good", "loss", "t_cam_obj"]        # the reference's four keys
    opt.reconstruct_objects([eye] * 2, [pts] * 2, [rays] * 2, [depth] * 2, unknowns=[["pose"], ["code"]])
    assert eng.kw["unknowns"] == [["pose"], ["code"]]
    got = opt.reconstruct_object_multiview(eye, views, unknowns=["translation", "rotation", "code"])
    assert eng.kw["unknowns"] == ["translation", "rotation", "code"] and sorted(got.keys()) == ["code", "is_good", "loss", "t_cam_obj"]
    assert isinstance(opt.estimate_pose_cam_obj(eye, 1.0, pts, np.zeros(64, F32), unknowns=["translation", "yaw"]), torch.Tensor)
    assert eng.kw["unknowns"] == ["translation", "yaw"]
    mask = E.unknowns_mask(["code"])
    opt.reconstruct_object(eye, pts, rays, depth, unknowns=mask)
    assert eng.kw["unknowns"] is mask
    # the config keys
    cfg = _config()
    cfg["optimizer"]["joint_optim"]["unknowns"] = ["translation", "yaw", "scale", "code"]
    cfg["optimizer"]["pose_only_optim"]["unknowns"] = ["translation", "yaw"]
    opt, eng = make(cfg)
    assert opt.unknowns_joint == ["translation", "yaw", "scale", "code"] and opt.unknowns_pose_only == ["translation", "yaw"]
    got = opt.reconstruct_object(eye, pts, rays, depth)
    assert eng.kw["unknowns"] == ["translation", "yaw", "scale", "code"] and sorted(got.keys()) == ["code", "is_good", "loss", "t_cam_obj"]
    opt.reconstruct_object_multiview(eye, views)
    assert eng.kw["unknowns"] == ["translation", "yaw", "scale", "code"]
    opt.estimate_pose_cam_obj(eye, 1.0, pts, np.zeros(64, F32))
    assert eng.kw["unknowns"] == ["translation", "yaw"]
    opt.reconstruct_object(eye, pts, rays, depth, unknowns=["code"])               # the call's keyword wins
    assert eng.kw["unknowns"] == ["code"]
    # one name as a string; an unknown name raises at construction
    cfg = _config()
    cfg["optimizer"]["joint_optim"]["unknowns"] = "pose"
    assert make(cfg)[0].unknowns_joint == ["pose"]
    for where in ("joint_optim", "pose_only_optim"):
        cfg = _config()
        cfg["optimizer"][where]["unknowns"] = ["pose", "shape"]
        with pytest.raises(ValueError):
            make(cfg)


def test_engine_calls_set_the_mask_on_the_resident_batch(monkeypatch):
    """unknowns= makes the Engine's one-call forms run a resident batch and set the mask in front of the run."""
    calls = []

    class FakeBatch(object):
        def __init__(self, *a, **k):
            pass

        def set_unknowns(self, live=None):
            calls.append(("unknowns", live))

        def run(self):
            calls.append(("run",))

        def results(self):
            return (np.zeros((1, 4, 4), F32), 2, 3, 4)

        def close(self):
            calls.append(("close",))
    monkeypatch.setattr(E, "Batch", FakeBatch)
    monkeypatch.setattr(E, "MultiviewBatch", FakeBatch)
    eng = E.Engine.__new__(E.Engine)
    eng.code_len = 64
    eng.pose_batch = lambda *a, **k: FakeBatch()
    one = [np.zeros((2, 3), F32)]
    eng.reconstruct_batch(None, [np.eye(4)], one, one, [np.zeros(2, F32)], unknowns=["pose"])
    assert calls == [("unknowns", ["pose"]), ("run",), ("close",)]
    del calls[:]
    eng.reconstruct_multiview_batch(None, [np.eye(4)], [[dict(t_ref_cam=np.eye(4), pts=one[0], rays=one[0], depth=np.zeros(2, F32))]], unknowns=["code"])
    assert calls == [("unknowns", ["code"]), ("run",), ("close",)]
    del calls[:]
    out = eng.estimate_pose_batch(None, [np.eye(4)], [1.0], one, [np.zeros(64, F32)], unknowns=["yaw"])
    assert calls == [("unknowns", ["yaw"]), ("run",), ("close",)] and out.shape == (1, 4, 4)
    eng._h = None


def test_tool_flag():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import reoptimise_map as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    p = inspect.signature(tool.reoptimise).parameters
    assert "unknowns" in p and p["unknowns"].default is None
    src = open(os.path.join(ROOT, "tools", "reoptimise_map.py")).read()
    assert '"--unknowns"' in src and "set_unknowns" in src
    with pytest.raises(ValueError):
        tool.reoptimise([], None, [], [], 64, unknowns=["poze"])


# ---- the conditioned fp64 reference ----------------------------------------------------------------------------------------------------
def _random_mask(seed, n=71, p=0.5):
    m = (np.random.default_rng(seed).random(n) >= p).astype(np.uint8)
    m[0], m[1] = 1, 0                     # both kinds present
    return m


@pytest.fixture(scope="module")
def small_lin():
    return _state("golden_recon_small.npz", 0)[-1]


def test_all_live_returns_the_input_bit_for_bit(small_lin):
    before = copy.deepcopy(small_lin)
    got = U.condition(small_lin, np.ones(71, np.uint8))
    assert sorted(got) == sorted(small_lin)
    for k, v in small_lin.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)) and np.asarray(got[k]).dtype == np.asarray(v).dtype, k
        assert np.array_equal(np.asarray(v), np.asarray(before[k])), k             # and the input is left alone
    got = U.condition(small_lin, _random_mask(4))
    for k, v in small_lin.items():
        assert np.array_equal(np.asarray(v), np.asarray(before[k])), k


@pytest.mark.parametrize("mask", ["code", "pose", "scale", "w_xz", "random", "none"])
def test_conditioned_system(small_lin, mask):
    live = {"code": 1 - E.unknowns_mask("code"), "pose": 1 - E.unknowns_mask("pose"), "scale": 1 - E.unknowns_mask("scale"),
            "w_xz": E.unknowns_mask(["translation", "yaw", "scale", "code"]), "random": _random_mask(5), "none": np.zeros(71, np.uint8)}[mask]
    lv = live.astype(bool)
    lin = small_lin
    got = U.condition(lin, live)
    h, b, dx = got["H"], got["b"], got["dx"]
    # live x live untouched, identity and zero elsewhere
    assert np.array_equal(h[np.ix_(lv, lv)], lin["H"][np.ix_(lv, lv)]) and np.array_equal(b[lv], lin["b"][lv])
    assert np.array_equal(h[~lv][:, ~lv], np.eye(int((~lv).sum()))) and not h[np.ix_(lv, ~lv)].any() and not h[np.ix_(~lv, lv)].any() and not b[~lv].any()
    assert not dx[~lv].any()
    # dx solves the FULL pinned system to fp64 round-off
    res = np.abs(h @ dx - b)
    bound = 64 * np.finfo(np.float64).eps * (np.abs(h) @ np.abs(dx) + np.abs(b))
    print("mask %s: %d live, worst |H dx - b| / (|H||dx| + |b|) = %.2e eps" % (mask, lv.sum(), float((res / np.maximum(bound / 64, 1e-300)).max()) if lv.any() else 0.0))
    assert np.all(res <= bound)
    if lv.any() and not lv.all():
        assert np.array_equal(dx[lv], np.linalg.solve(lin["H"][np.ix_(lv, lv)], lin["b"][lv]))
    # every scale and allowance of the metric vanishes at a frozen entry
    for k in U.MATRICES:
        assert not got[k][~lv].any() and not got[k][:, ~lv].any(), k
        assert np.array_equal(got[k][np.ix_(lv, lv)], lin[k][np.ix_(lv, lv)]), k
    for k in U.VECTORS:
        assert not got[k][~lv].any() and np.array_equal(got[k][lv], lin[k][lv]), k
    assert not got["j_rot"][~lv[:7]].any()
    # the metric accepts the reference itself and refuses a frozen dx that is not exactly zero
    import gn_metric as M
    own = dict(H=h.astype(F32), b=b.astype(F32), dx=dx.astype(F32))
    assert M.within_tau(M.scaled_errors(own, got, 1e7))
    if not lv.all():
        off = dict(own, dx=own["dx"].copy())
        off["dx"][np.nonzero(~lv)[0][0]] = F32(1e-30)
        assert not M.within_tau(M.scaled_errors(off, got, 1e7))


def test_conditioned_posterior(small_lin):
    lam = small_lin["H"] - small_lin["H_damp"]
    live = _random_mask(6)
    lv = live.astype(bool)
    cl, cg = U.condition_lambda(lam, small_lin["b"], live)
    assert not cl[~lv].any() and not cl[:, ~lv].any() and not cg[~lv].any() and np.array_equal(cl[np.ix_(lv, lv)], lam[np.ix_(lv, lv)])
    emu, ref = U.posterior(lam, live), U.posterior(lam, live, refined=True)
    assert emu["status"] == 0
    pl, cdl = lv[:7], lv[7:]
    for rec in (emu, ref):
        assert not rec["info_pose"][~pl].any() and not rec["info_pose"][:, ~pl].any() and not rec["cov_pose"][~pl].any() and not rec["var_code"][~cdl].any()
        assert np.all(rec["var_code"][cdl] > 0)
    for k in ("info_pose", "cov_pose", "var_code"):
        assert R.rel_err(emu[k], ref[k]) <= 1e-9, k
    # the Schur complement over the LIVE code entries on the live pose entries, stated directly
    p, c = np.nonzero(pl)[0], 7 + np.nonzero(cdl)[0]
    schur = lam[np.ix_(p, p)] - lam[np.ix_(p, c)] @ np.linalg.solve(lam[np.ix_(c, c)], lam[np.ix_(c, p)])
    assert R.rel_err(ref["info_pose"][np.ix_(p, p)], schur) <= 1e-9
    # no pose entry live: both pose blocks all zero, status OK; nothing live: everything zero
    rec = U.posterior(lam, E.unknowns_mask("code"))
    assert rec["status"] == 0 and not rec["info_pose"].any() and not rec["cov_pose"].any() and np.all(rec["var_code"] > 0)
    rec = U.posterior(lam, np.zeros(71, np.uint8))
    assert rec["status"] == 0 and not rec["info_pose"].any() and not rec["cov_pose"].any() and not rec["var_code"].any()
    # all live: posterior_ref.sweep itself
    full = R.sweep(lam, 7)
    rec = U.posterior(lam, np.ones(71, np.uint8))
    assert all(np.array_equal(rec[k], full[k]) for k in ("info_pose", "cov_pose", "var_code"))


# ---- the exactness argument, on the emulated elimination -------------------------------------------------------------------------------
def _lds(h, b):
    n = h.shape[0]
    a = np.full((NS1, LDA), np.nan)          # LDS as the assembly leaves it (tests/test_solve_schedule.py)
    a[:n, :n] = h
    a[:n, n] = b
    a[n, :n] = b
    return a


@pytest.mark.parametrize("mask", ["code", "pose", "scale", "w_xz", "random", "none"])
def test_a_pinned_system_solves_to_exact_zeros_and_the_reduced_system(small_lin, mask):
    """The panel schedule (per_panel: the kernel's, lane for lane) and the per-pivot rows-in-lanes schedule (solve_emulator) on the pinned
    71 x 71 system: dx_i == 0.0 exactly at every frozen i, and the live entries are, bit for bit, the emulation of the REDUCED system
    padded back -- the reduced system's entries see the same multiply-subtracts in the same pivot order."""
    live = {"code": 1 - E.unknowns_mask("code"), "pose": 1 - E.unknowns_mask("pose"), "scale": 1 - E.unknowns_mask("scale"),
            "w_xz": E.unknowns_mask(["translation", "yaw", "scale", "code"]), "random": _random_mask(7), "none": np.zeros(71, np.uint8)}[mask]
    lv = live.astype(bool)
    h, b = U.pin(small_lin["H"], small_lin["b"], live)
    with np.errstate(invalid="ignore"):
        panel = per_panel(_lds(h, b), 71)
        pivot, sing = S.solve_rows_in_lanes(h, b)
    assert not sing and np.isfinite(panel).all()
    assert np.array_equal(panel[~lv], np.zeros(int((~lv).sum()))) and np.array_equal(pivot[~lv], np.zeros(int((~lv).sum())))
    if lv.any():
        with np.errstate(invalid="ignore"):
            red, sing = S.solve_rows_in_lanes(small_lin["H"][np.ix_(lv, lv)], small_lin["b"][lv])
        assert not sing
        assert np.array_equal(pivot[lv], red)
        # per_panel's reciprocal is 1 / d, solve_emulator's a refined single-precision one: same schedule, its own bits
        ref = np.linalg.solve(small_lin["H"][np.ix_(lv, lv)], small_lin["b"][lv])
        assert np.abs(panel[lv] - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max())
        assert np.abs(red - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max())
    # pose-only width: 6 x 6 with w_x, w_z frozen
    rng = np.random.default_rng(8)
    j = rng.standard_normal((50, 6))
    h6, b6 = j.T @ j / 50 + 1e-2 * np.eye(6), rng.standard_normal(6)
    l6 = np.array([1, 1, 1, 0, 1, 0], bool)
    hp, bp = U.pin(h6, b6, l6)
    with np.errstate(invalid="ignore"):
        d6 = per_panel(_lds(hp, bp), 6)
        r6, _ = S.solve_rows_in_lanes(hp, bp)
        q6, _ = S.solve_rows_in_lanes(h6[np.ix_(l6, l6)], b6[l6])
    assert np.array_equal(d6[~l6], [0.0, 0.0]) and np.array_equal(r6[~l6], [0.0, 0.0]) and np.array_equal(r6[l6], q6)
