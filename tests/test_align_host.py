"""CPU-only: map alignment (dsp_map_align, include/dsp_gn.h) above and below the device.

  * every new symbol is declared in the header, exported by the library and bound in dsp_slam_amd/_lib.py; the ABI version stays 6;
  * dsp_debug_align_rows (csrc/align_math.h: the rows and the written summation tree the device kernels run) against the numpy restatement
    (tests/align_ref.py), bit for bit;
  * dsp_debug_align_step against the restatement: xi bit for bit, T_trial to 1e-14 (sin / cos may differ in the last place);
  * the refusals that need no device (dsp_debug_align_check: the checks dsp_map_align makes before it touches the device);
  * the ALGORITHM in float64 with the oracle's decoder on a three-object scene: convergence from 5 degrees / 0.05, and a 30 degrees / 0.3
    hypothesis that ends in a local minimum -- the reason hypotheses are part of the interface.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_ref as A
import query_ref as Q
from conftest import ROOT
from dsp_slam_amd import _lib as L
from dsp_slam_amd import map_objects as M

F32, F64 = np.float32, np.float64
NEW = ["dsp_align_params_default", "dsp_map_align", "dsp_map_align_last_stats", "dsp_debug_align_rows", "dsp_debug_align_step", "dsp_debug_align_check"]
E_ARG = -1
HUBER, MAX_DIST = float(F32(0.05)), float(F32(0.3))        # float32 values, so that a float32 |d| can equal them exactly


def _u64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    for name, val in (("DSP_ALIGN_OK", L.ALIGN_OK), ("DSP_ALIGN_CONVERGED", L.ALIGN_CONVERGED), ("DSP_ALIGN_NO_SUPPORT", L.ALIGN_NO_SUPPORT),
                      ("DSP_ALIGN_SINGULAR", L.ALIGN_SINGULAR), ("DSP_ALIGN_RECORD", L.ALIGN_RECORD), ("DSP_ALIGN_TRACE", L.ALIGN_TRACE)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src), name
    assert (A.OK, A.CONVERGED, A.NO_SUPPORT, A.SINGULAR) == (L.ALIGN_OK, L.ALIGN_CONVERGED, L.ALIGN_NO_SUPPORT, L.ALIGN_SINGULAR)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dsp_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    bound = {n for n, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert lib.dsp_abi_version() == 6
    # the struct as the header lays it out, and the defaults
    fields = re.search(r"typedef struct dsp_align_params \{(.*?)\} dsp_align_params;", src, flags=re.S).group(1)
    names = [n for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", fields) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [n for n, _ in L.AlignParams._fields_]
    p = L.AlignParams()
    lib.dsp_align_params_default(C.byref(p))
    got = {n: getattr(p, n) for n in names}
    want = dict(A.DEFAULTS)
    want.pop("step_control")
    want.update(lambda0=0.0, up=0.0, down=0.0, lambda_min=0.0, lambda_max=0.0)
    assert got == want


# ---- 1. rows and the tree, bit for bit ---------------------------------------------------------------------------------------------------
def _row_inputs(rng, n):
    pw = rng.uniform(-3, 3, (n, 3)).astype(F32)
    obj = rng.integers(-1, 3, n).astype(np.int32)
    dist = (rng.uniform(-0.5, 0.5, n) * 10.0 ** rng.uniform(-4, 0, n)).astype(F32)
    g = (rng.normal(size=(n, 3)) * rng.uniform(0.2, 2.0, (n, 1))).astype(F32)
    w = rng.uniform(0, 2, n).astype(F32)
    special = [("dist", F32(HUBER)), ("dist", F32(-HUBER)), ("dist", F32(MAX_DIST)), ("dist", F32(-MAX_DIST)),
               ("dist", np.nextafter(F32(MAX_DIST), F32(1))), ("dist", np.nextafter(F32(HUBER), F32(1))), ("dist", F32(np.inf)), ("dist", F32(np.nan)),
               ("pw", F32(np.nan)), ("g", F32(np.nan)), ("g", F32(np.inf)), ("w", F32(0)), ("obj", -1), ("pw", F32(np.inf))]
    # every special case in turn at random points (all of them once n allows it); the rest stays a mix of inside / outside the gate
    for k, i in enumerate(rng.permutation(n)[:max(1, min(n // 2, 3 * len(special)))]):
        what, v = special[k % len(special)] if n > 1 else ("dist", F32(HUBER))
        if what == "dist":
            dist[i] = v
            obj[i] = max(obj[i], 0)
        elif what == "pw":
            pw[i, k % 3] = v
        elif what == "g":
            g[i, k % 3] = v
            obj[i] = max(obj[i], 0)
        elif what == "w":
            w[i] = v
        else:
            obj[i] = v
    return pw, obj, dist, g, w


def host_rows(pw, obj, dist, g, w, huber=HUBER, max_dist=MAX_DIST):
    sums = np.full(A.NSUM, 7.0, F64)
    rc = L.load().dsp_debug_align_rows(pw.shape[0], L.ptr(pw), L.ptr(obj, L.c_i32p), L.ptr(dist), L.ptr(g), L.ptr(w), huber, max_dist, L.ptr(sums, L.c_f64p))
    return rc, sums


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_rows_and_tree_are_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    pw, obj, dist, g, w = _row_inputs(rng, n)
    for weights in (w, None):
        rc, sums = host_rows(pw, obj, dist, g, weights)
        want = A.tree_sum(A.row_terms(pw, obj, dist, g, weights, HUBER, MAX_DIST))
        assert rc == 0 and np.array_equal(_u64(sums), _u64(want)), (n, sums - want)
    if n >= 257:
        terms = A.row_terms(pw, obj, dist, g, w, HUBER, MAX_DIST)
        used = terms[:, A.IDX_N] == 1
        valid = terms[:, A.IDX_W] > 0
        assert used.sum() > n // 4 and (valid & ~used).sum() > 10 and (~valid).sum() >= 5
        # the mix: both sides of the Huber width and of the gate, and both equalities, among the used / valid points
        a = np.abs(dist.astype(F64))
        assert (used & (a < HUBER)).any() and (used & (a > HUBER)).any() and (used & (a == HUBER)).any() and (used & (a == MAX_DIST)).any()
        assert (valid & ~used & (a > MAX_DIST)).any() and (valid & ~used & (obj < 0)).any()
        # a valid point that is not used contributes the constant and a zero row
        k = np.flatnonzero(valid & ~used)[0]
        assert terms[k, A.IDX_COST] == float(w[k]) * HUBER * (2 * MAX_DIST - HUBER) and not terms[k, :A.IDX_COST].any()
        assert np.allclose(host_rows(pw, obj, dist, g, w)[1], terms.sum(0), rtol=1e-12, atol=1e-12)        # and the tree is a sum


def test_rows_refuse_a_bad_gate():
    pw, obj, dist, g, w = _row_inputs(np.random.default_rng(5), 8)
    assert host_rows(pw, obj, dist, g, w, huber=0.4, max_dist=0.3)[0] == E_ARG
    assert host_rows(pw, obj, dist, g, w, huber=0.0)[0] == E_ARG
    assert host_rows(pw, obj, dist, g, w, max_dist=np.inf)[0] == E_ARG
    rc, sums = host_rows(pw[:0], obj[:0], dist[:0], g[:0], None)
    assert rc == 0 and not sums.any()


# ---- 2. the step -------------------------------------------------------------------------------------------------------------------------
def host_step(H, b, damp, lam, T):
    H, b, T = np.ascontiguousarray(H, F64), np.ascontiguousarray(b, F64), np.ascontiguousarray(T, F64)
    xi, Tt, st = np.full(6, 7.0, F64), np.full((4, 4), 7.0, F64), C.c_int32(-5)
    rc = L.load().dsp_debug_align_step(L.ptr(H, L.c_f64p), L.ptr(b, L.c_f64p), damp, lam, L.ptr(T, L.c_f64p), C.byref(st), L.ptr(xi, L.c_f64p),
                                       L.ptr(Tt, L.c_f64p))
    return rc, st.value, xi, Tt


def _close14(a, b):
    return bool(np.all(np.abs(a - b) <= 1e-14 * np.maximum(1.0, np.abs(b))))


def test_step_is_the_restatement():
    rng = np.random.default_rng(7)
    for case in range(40):
        J = rng.normal(size=(30, 6)) * 10.0 ** rng.uniform(-1, 1, 6)
        H = J.T @ J
        H = (H + H.T) / 2
        target = rng.normal(size=6)
        target *= rng.uniform(0, 1) / np.sqrt((target * target).sum())          # |xi| <= 1
        if case % 4 == 0:
            target[3:] *= 1e-7                                                  # the theta -> 0 branch
        b = H @ target
        damp, lam = (0.0, 0.0) if case % 2 or case % 4 == 0 else (1e-6, 10.0 ** rng.uniform(-6, -2))
        T = A.rigid(Q.random_rotations(rng, 1)[0], rng.uniform(-5, 5, 3))
        rc, st, xi, Tt = host_step(H, b, damp, lam, T)
        want = A.solve(H, b, damp, lam)
        assert rc == 0 and st == A.OK and np.array_equal(_u64(xi), _u64(want)), case
        if case % 4 == 0:
            assert (xi[3:] ** 2).sum() < A.SMALL_TH2
        assert np.sqrt((xi * xi).sum()) <= 1.0 + 1e-3
        assert _close14(Tt, A.apply_step(want, T)), case
        assert np.array_equal(Tt[3], [0, 0, 0, 1])
        # and it is the step: exp(xi) T, against the matrix exponential's series
        X = np.zeros((4, 4))
        X[:3, :3] = [[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]]
        X[:3, 3] = xi[:3]
        E, term = np.eye(4), np.eye(4)
        for k in range(1, 30):
            term = term @ X / k
            E = E + term
        assert np.abs(Tt - E @ T).max() < 1e-12
    # only the upper triangle is read
    H2 = np.triu(H) + np.tril(np.full((6, 6), 99.0), -1)
    assert np.array_equal(_u64(host_step(H2, b, damp, lam, T)[2]), _u64(xi))


def test_step_reports_a_singular_system():
    T = np.eye(4)
    b = np.ones(6)
    for H in (np.zeros((6, 6)), -np.eye(6), np.diag([1.0, 1, 1, 1, 1, np.nan]), np.outer(np.ones(6), np.ones(6))):
        rc, st, xi, Tt = host_step(H, b, 0.0, 0.0, T)
        assert rc == 0 and st == A.SINGULAR and A.solve(H, b, 0.0, 0.0) is None
        assert np.all(xi == 7.0) and np.all(Tt == 7.0)                          # untouched
    # damping makes the zero matrix solvable: xi = b / (damp + lambda)
    rc, st, xi, _ = host_step(np.zeros((6, 6)), b, 0.125, 0.125, T)
    assert st == A.OK and np.array_equal(xi, np.full(6, 4.0))


# ---- 3. refusals that need no device -----------------------------------------------------------------------------------------------------
def _check(T0=None, w=None, n_pts=0, **fields):
    p = L.AlignParams()
    L.load().dsp_align_params_default(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    T0 = np.ascontiguousarray(np.eye(4)[None] if T0 is None else T0, F64).reshape(-1, 4, 4)
    w = None if w is None else L.f32(w)
    return L.load().dsp_debug_align_check(C.byref(p), L.ptr(T0, L.c_f64p), T0.shape[0], L.ptr(w), n_pts if w is None else w.shape[0])


def test_refused_parameters_and_poses():
    assert _check() == 0
    assert _check(lambda0=1e-3, up=4.0, down=0.5, lambda_min=1e-9, lambda_max=1e6) == 0
    for bad in (dict(iterations=0), dict(min_points=5), dict(huber=0.4, max_dist=0.3), dict(huber=0.0), dict(huber=-1.0), dict(max_dist=np.inf),
                dict(huber=np.nan), dict(damp=-1e-9), dict(damp=np.inf), dict(trans_tol=-1.0), dict(rot_tol=np.nan),
                dict(lambda0=1e-3), dict(lambda0=1e-3, up=1.0, down=0.5, lambda_min=1e-9, lambda_max=1e6),
                dict(lambda0=1e-3, up=4.0, down=0.5, lambda_min=1e-3, lambda_max=1e-6)):
        assert _check(**bad) == E_ARG, bad
    assert _check(huber=0.3, max_dist=0.3) == 0
    rng = np.random.default_rng(9)
    good = A.rigid(Q.random_rotations(rng, 1)[0], [1.0, -2.0, 3.0])
    assert _check(T0=good) == 0 and A.check_pose(good)
    bad_poses = []
    for s in (1.001, 0.999, 2.0):                     # a scaled pose: off 1 by more than 1e-4
        p = good.copy(); p[:3, :3] *= s; bad_poses.append(p)
    p = good.copy(); p[0, 1] += 0.01; bad_poses.append(p)                   # not a rotation
    p = good.copy(); p[3, 3] = 2.0; bad_poses.append(p)
    p = good.copy(); p[3, 0] = 1e-30; bad_poses.append(p)
    p = good.copy(); p[1, 3] = np.nan; bad_poses.append(p)
    p = good.copy(); p[1, 3] = 1e39; bad_poses.append(p)                    # not finite in float32
    bad_poses.append(np.zeros((4, 4)))
    for p in bad_poses:
        assert _check(T0=p) == E_ARG and not A.check_pose(p)
        assert _check(T0=np.stack([good, p])) == E_ARG                       # anywhere in the list
    p = good.copy(); p[:3, :3] *= 1.00005                                    # inside the tolerance
    assert _check(T0=p) == 0 and A.check_pose(p)
    assert _check(T0=np.zeros((0, 4, 4))) == 0
    assert _check(w=[1.0, 0.0, 2.0]) == 0
    for w in ([1.0, -1e-9], [np.nan], [np.inf]):
        assert _check(w=w) == E_ARG
    assert _check(T0=np.stack([good] * 3), n_pts=(2 ** 31 - 1) // 3) == 0 and _check(T0=np.stack([good] * 3), n_pts=(2 ** 31 - 1) // 3 + 1) == E_ARG
    # without a handle the call itself refuses, whatever else it is given
    assert L.load().dsp_map_align(None, None, None, 0, None, None, 0, None, 0, None, None, None, None, None, None) == E_ARG
    assert L.load().dsp_map_align_last_stats(None, None) == E_ARG


def test_localise_adds_ids_on_a_hand_built_result():
    class Fake:
        def align_to_map(self, poses, codes, pts, t0, weights=None, trace=False, per_point=False, **params):
            assert per_point and poses.shape == (2, 4, 4) and len(codes) == 2 and params == {"iterations": 3}
            return {"obj": np.array([[0, 1, -1], [1, 1, 0]], np.int32), "dist": np.zeros((2, 3), F32), "best": 0}
    objs = [dict(id=17, pose=np.eye(4), code=np.zeros(64, F32)), dict(id=4, pose=np.eye(4), code=np.zeros(64, F32))]
    res = M.localise(Fake(), objs, np.zeros((3, 3)), np.eye(4), iterations=3)
    assert res["id"].tolist() == [[17, 4, -1], [4, 4, 17]] and res["best"] == 0


# ---- 4. the algorithm, float64, oracle decoder -------------------------------------------------------------------------------------------
SEED = 7


def _oracle_scene(dec):
    """Three objects whose spheres do not overlap, 100 points per object on the decoder's zero set (float64 Newton projection along the
    gradient, kept where |sdf| < 1e-6 and |p_o| < 0.9), moved to a sensor frame by a fixed T_true."""
    from oracle import dsp_oracle
    rng = np.random.default_rng(SEED)
    t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [2.6, 0.3, -0.2], [4.0, -3.0, 1.0]])
    codes = rng.uniform(-0.3, 0.3, (3, 64)).astype(F32)
    decode = lambda o, p: (lambda y, g, _: (y, g[:, -3:]))(*dsp_oracle._decode64(dec, codes[o].astype(F64), np.asarray(p, F64)))
    world = []
    for o in range(3):
        p = rng.normal(size=(400, 3))
        p *= (0.5 * rng.uniform(0, 1, (400, 1)) ** (1 / 3)) / np.sqrt((p * p).sum(1))[:, None]
        for _ in range(12):
            y, g = decode(o, p)
            step = -(y / np.maximum((g * g).sum(1), 1e-12))[:, None] * g
            norm = np.sqrt((step * step).sum(1))[:, None]
            p = p + step * np.minimum(1.0, 0.1 / np.maximum(norm, 1e-30))
        y, _ = decode(o, p)
        keep = p[(np.abs(y) < 1e-6) & (np.sqrt((p * p).sum(1)) < 0.9)][:100]
        assert keep.shape[0] == 100
        tw = t[o].astype(F64)
        world.append(keep @ tw[:3, :3].T + tw[:3, 3])
    world = np.concatenate(world)
    T_true = A.rigid(A.axis_angle([0.3, -1.0, 0.5], 0.7), [0.5, -1.5, 2.0])
    inv = np.linalg.inv(T_true)
    return dict(map=A.Map(t, codes), decode=decode, pts=world @ inv[:3, :3].T + inv[:3, 3], T_true=T_true, centre=world.mean(0))


def test_algorithm_converges_and_needs_hypotheses(oracle_decoder):
    s = _oracle_scene(oracle_decoder)
    rng = np.random.default_rng(SEED)
    near, far = A.offset_pose(rng, s["T_true"], 5.0, 0.05, s["centre"]), A.offset_pose(rng, s["T_true"], 30.0, 0.3, s["centre"])
    kw = dict(max_dist=0.3, huber=0.05, trans_tol=0.0, rot_tol=0.0, evaluate=A.evaluate64)
    r = A.run(near, s["pts"], None, s["map"], s["decode"], iterations=6, **kw)
    tr = r["trace"]
    assert tr[0]["n_used"] == 300                                             # all points used at the first evaluation
    costs = [e["cost"] for e in tr]
    assert len(costs) == 6 and all(b < a for a, b in zip(costs, costs[1:])), costs          # the cost falls at every step
    et, er = A.pose_error(r["pose"], s["T_true"])
    assert et < 1e-9 and er < 1e-9, (et, er)                                  # within six evaluations
    r2 = A.run(far, s["pts"], None, s["map"], s["decode"], iterations=12, **kw)
    assert r2["cost"] >= 100 * r["cost"], (r2["cost"], r["cost"])
    results = [r, r2]
    ok = [k for k, x in enumerate(results) if x["n_used"] >= 6]
    assert min(ok, key=lambda k: results[k]["cost"]) == 0                     # best == 0
    # the pipeline's evaluation (float32 points, transform and decoder values, as the device computes them) runs the same loop to the same
    # place: its pose differs from the float64 algorithm's by float32 roundings of coordinates of size <= 6, i.e. by far less than 1e-5
    dec32 = lambda o, p: tuple(np.asarray(a, F32) for a in s["decode"](o, p))
    r32 = A.run(near, s["pts"].astype(F32), None, s["map"], dec32, iterations=6, max_dist=0.3, huber=0.05, trans_tol=0.0, rot_tol=0.0)
    et, er = A.pose_error(r32["pose"], s["T_true"])
    assert r32["trace"][0]["n_used"] == 300 and et < 1e-5 and er < 1e-5, (et, er)
