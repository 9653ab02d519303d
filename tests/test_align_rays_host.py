"""CPU-only: ray alignment (dsp_map_align_rays, include/dsp_gn.h) above and below the device.

  * every new symbol is declared in the header, exported by the library and bound in dsp_slam_amd/_lib.py; the ABI version stays 6;
  * dsp_debug_align_ray_rows (csrc/align_rays_math.h: the residual and the match the device kernels run, then align_math.h's rows and tree)
    against the numpy restatement (tests/align_rays_ref.py), bit for bit;
  * the refusals that need no device (dsp_debug_align_rays_check: the checks dsp_map_align_rays makes before it touches the device);
  * the ALGORITHM in float64 -- float64 rays, a float64 sphere tracer, the oracle's decoder -- through align_ref.run on a three-object
    scene seen by a few dozen rays: recovery from 5 and from 20 degrees, where the point evaluation's basin ends;
  * map_objects.localise_rays / localise_depth on a hand-built engine.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_rays_ref as AR
import align_ref as A
import query_ref as Q
from conftest import ROOT
from dsp_slam_amd import _lib as L
from dsp_slam_amd import map_objects as M

F32, F64 = np.float32, np.float64
NEW = ["dsp_map_align_rays", "dsp_map_align_rays_last_stats", "dsp_debug_align_ray_rows", "dsp_debug_align_rays_check", "dsp_align_rays_default_max_gap"]
E_ARG = -1
HUBER, MAX_DIST, MAX_GAP = float(F32(0.05)), float(F32(0.3)), float(F32(0.5))      # float32 values, so that a float32 gap can equal the gate


def _u64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dsp_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    bound = {n for n, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert lib.dsp_abi_version() == 6
    p = L.AlignParams()
    lib.dsp_align_params_default(C.byref(p))
    assert lib.dsp_align_rays_default_max_gap(C.byref(p)) == 2.0 * p.max_dist and lib.dsp_align_rays_default_max_gap(None) == 0.0
    assert lib.dsp_map_align_rays(None, None, None, 0, None, None, None, 0, None, 0, None, None, 1.0, None, None, None, None, None, None, None) == E_ARG
    assert lib.dsp_map_align_rays_last_stats(None, None) == E_ARG


# ---- 1. residual, match, rows and tree, bit for bit --------------------------------------------------------------------------------------
def _ray_inputs(rng, n):
    ow = rng.uniform(-2, 2, (n, 3)).astype(F32)
    u = rng.normal(size=(n, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    pw = (ow + u * rng.uniform(1.0, 3.5, (n, 1))).astype(F32)
    with np.errstate(all="ignore"):
        length = np.sqrt(Q.norm2((pw - ow).astype(F32))).astype(F32)
    obj = rng.integers(-1, 3, n).astype(np.int32)
    # gaps on both sides of the gate and of max_dist
    t_hit = (length - (rng.uniform(-0.8, 0.8, n) * 10.0 ** rng.uniform(-3, 0, n)).astype(F32)).astype(F32)
    dist_hit = (rng.uniform(-1e-3, 1e-3, n)).astype(F32)
    status = np.where(obj < 0, AR.MISS, AR.HIT).astype(np.int32)
    gw = (rng.normal(size=(n, 3)) * rng.uniform(0.2, 2.0, (n, 1))).astype(F32)
    w = rng.uniform(0, 2, n).astype(F32)
    special = ["at", "inside", "outside", "at_neg", "miss", "undecided", "void", "nan_point", "w0", "g_nan", "g_inf", "no_winner", "t_inf", "nan_origin"]
    for k, i in enumerate(rng.permutation(n)[:max(1, min(n // 2, 3 * len(special)))]):
        what = special[k % len(special)] if n > 1 else "at"
        if what in ("at", "inside", "outside", "at_neg"):
            obj[i], status[i] = max(obj[i], 0), AR.HIT
            g = F32(MAX_GAP)
            t_hit[i] = length[i] - g if what != "at_neg" else length[i] + g
            if what == "inside":
                t_hit[i] = np.nextafter(t_hit[i], F32(np.inf))
            if what == "outside":
                t_hit[i] = np.nextafter(t_hit[i], F32(-np.inf))
        elif what == "miss":
            obj[i], status[i], t_hit[i], dist_hit[i] = -1, AR.MISS, np.inf, np.inf
        elif what == "undecided":
            obj[i], status[i] = max(obj[i], 0), AR.UNDECIDED
        elif what == "void":
            pw[i] = ow[i]
        elif what == "nan_point":
            pw[i, k % 3] = np.nan
        elif what == "nan_origin":
            ow[i, k % 3] = np.nan
        elif what == "w0":
            w[i] = 0
        elif what == "g_nan":
            gw[i, k % 3], obj[i], status[i] = np.nan, max(obj[i], 0), AR.HIT
        elif what == "g_inf":
            gw[i, k % 3], obj[i], status[i] = np.inf, max(obj[i], 0), AR.HIT
        elif what == "no_winner":
            obj[i], status[i], t_hit[i], dist_hit[i] = -1, AR.UNDECIDED, np.inf, np.inf
        else:
            obj[i], status[i], t_hit[i] = max(obj[i], 0), AR.HIT, np.inf
    return ow, pw, obj, t_hit, dist_hit, status, gw, w


def host_ray_rows(ow, pw, obj, t_hit, dist_hit, status, gw, w, huber=HUBER, max_dist=MAX_DIST, max_gap=MAX_GAP):
    n = pw.shape[0]
    obj_row, d, sums = np.full(n, 7, np.int32), np.full(n, 7.0, F32), np.full(A.NSUM, 7.0, F64)
    rc = L.load().dsp_debug_align_ray_rows(n, L.ptr(ow), L.ptr(pw), L.ptr(obj, L.c_i32p), L.ptr(t_hit), L.ptr(dist_hit), L.ptr(status, L.c_i32p), L.ptr(gw),
                                           L.ptr(w), huber, max_dist, max_gap, L.ptr(obj_row, L.c_i32p), L.ptr(d), L.ptr(sums, L.c_f64p))
    return rc, obj_row, d, sums


@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_ray_rows_are_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(200 + n)
    inp = _ray_inputs(rng, n)
    ow, pw, obj, t_hit, dist_hit, status, gw, w = inp
    for weights in (w, None):
        for gate in (MAX_GAP, np.inf, MAX_DIST):
            rc, obj_row, d, sums = host_ray_rows(*inp[:7], weights, max_gap=gate)
            want = AR.ray_rows(*inp[:7], weights, HUBER, MAX_DIST, gate)
            assert rc == 0 and np.array_equal(obj_row, want[0]) and np.array_equal(_u32(d), _u32(want[1])), (n, gate)
            assert np.array_equal(_u64(sums), _u64(want[2])), (n, gate, sums - want[2])
    if n == 300:
        obj_row, d, _ = AR.ray_rows(*inp, HUBER, MAX_DIST, MAX_GAP)
        free, _, _ = AR.ray_rows(*inp, HUBER, MAX_DIST, np.inf)
        with np.errstate(all="ignore"):
            gap = (np.sqrt(Q.norm2((pw - ow).astype(F32))).astype(F32) - t_hit).astype(F64)
        hit = (status == AR.HIT) & (obj >= 0)
        # the gate: equality on both sides is matched, the neighbouring float32 values fall on either side
        assert (hit & (gap == MAX_GAP) & (obj_row >= 0)).any() and (hit & (gap == -MAX_GAP) & (obj_row >= 0)).any()
        assert (hit & (gap > MAX_GAP) & (gap < MAX_GAP + 1e-6) & (obj_row < 0)).any()          # one float32 step of t_hit past the gate ...
        assert (hit & (gap < MAX_GAP) & (gap > MAX_GAP - 1e-6) & (obj_row >= 0)).any()         # ... and one inside it
        assert (obj_row >= 0).sum() > 60 and ((free >= 0) & (obj_row < 0)).sum() >= 4             # the gate takes rows out; +inf takes none of them
        void = AR.R.rays(ow, (pw - ow).astype(F32))[1]
        assert np.all(free[hit & ~void & np.isfinite(gap)] >= 0) and np.all(free[hit & ~np.isfinite(gap)] < 0)
        assert np.all(obj_row[status != AR.HIT] == -1) and (status == AR.UNDECIDED).sum() >= 4
        assert np.all(np.isposinf(d[obj < 0])) and np.all(obj_row[obj < 0] == -1)
        assert np.all(pw == ow, 1).any() and np.isnan(ow).any() and np.all(np.isposinf(d[void])) and np.all(obj_row[void] == -1)
        terms = A.row_terms(pw, obj_row, d, gw, w, HUBER, MAX_DIST)
        valid, used = terms[:, A.IDX_W] > 0, terms[:, A.IDX_N] == 1
        # an unmatched ray whose end point is finite costs w rho(max_dist); a void ray with a finite end point does too
        k = np.flatnonzero(valid & (obj_row < 0))
        assert k.size > 20 and np.all(terms[k, A.IDX_COST] == w[k].astype(F64) * HUBER * (2 * MAX_DIST - HUBER)) and not terms[k, :A.IDX_COST].any()
        assert (void & valid).any() and used.sum() > 30 and (~valid).sum() >= 4
        assert not used[~np.isfinite(gw).all(1)].any()


def test_ray_rows_refuse_bad_gates():
    inp = _ray_inputs(np.random.default_rng(5), 8)
    assert host_ray_rows(*inp, huber=0.4, max_dist=0.3)[0] == E_ARG
    assert host_ray_rows(*inp, max_dist=np.inf, max_gap=np.inf)[0] == E_ARG
    assert host_ray_rows(*inp, max_gap=np.nan)[0] == E_ARG
    assert host_ray_rows(*inp, max_gap=float(np.nextafter(MAX_DIST, 0.0)))[0] == E_ARG
    assert host_ray_rows(*inp, max_gap=MAX_DIST)[0] == 0
    rc, _, _, sums = host_ray_rows(*[x[:0] for x in inp[:7]], None)
    assert rc == 0 and not sums.any()


# ---- 2. refusals that need no device -----------------------------------------------------------------------------------------------------
def _check(T0=None, w=None, n_rays=0, n_obj=3, max_gap=1.0, raycast=None, **fields):
    lib = L.load()
    p, rp = L.AlignParams(), L.RaycastParams()
    lib.dsp_align_params_default(C.byref(p))
    lib.dsp_raycast_params_default(C.byref(rp))
    for k, v in fields.items():
        setattr(p, k, v)
    for k, v in (raycast or {}).items():
        setattr(rp, k, v)
    T0 = np.ascontiguousarray(np.eye(4)[None] if T0 is None else T0, F64).reshape(-1, 4, 4)
    w = None if w is None else L.f32(w)
    return lib.dsp_debug_align_rays_check(C.byref(p), C.byref(rp), max_gap, L.ptr(T0, L.c_f64p), T0.shape[0], L.ptr(w), n_rays if w is None else w.shape[0],
                                          n_obj)


def test_every_refusal():
    assert _check() == 0 and _check(max_gap=np.inf) == 0 and _check(max_gap=0.3) == 0
    # the gate
    for g in (np.nan, 0.0, -1.0, float(np.nextafter(0.3, 0.0)), -np.inf):
        assert _check(max_gap=g) == E_ARG, g
    assert _check(max_dist=0.5, max_gap=0.4) == E_ARG and _check(max_dist=0.5, max_gap=0.5) == 0
    # everything dsp_map_align refuses
    for bad in (dict(iterations=0), dict(min_points=5), dict(huber=0.4, max_dist=0.3), dict(huber=0.0), dict(max_dist=np.inf), dict(damp=-1e-9),
                dict(trans_tol=-1.0), dict(rot_tol=np.nan), dict(lambda0=1e-3), dict(lambda0=1e-3, up=4.0, down=0.5, lambda_min=1e-3, lambda_max=1e-6)):
        assert _check(max_gap=np.inf, **bad) == E_ARG, bad
    good = A.rigid(Q.random_rotations(np.random.default_rng(9), 1)[0], [1.0, -2.0, 3.0])
    scaled, nan = good.copy(), good.copy()
    scaled[:3, :3] *= 1.001
    nan[1, 3] = np.nan
    assert _check(T0=good) == 0
    for p in (scaled, nan, np.zeros((4, 4))):
        assert _check(T0=p) == E_ARG and _check(T0=np.stack([good, p])) == E_ARG
    for w in ([1.0, -1e-9], [np.nan], [np.inf]):
        assert _check(w=w) == E_ARG
    assert _check(w=[1.0, 0.0, 2.0]) == 0
    # everything dsp_map_raycast refuses
    for bad in (dict(t_min=-1.0), dict(t_min=2.0, t_max=1.0), dict(eps=0.0), dict(eps=np.inf), dict(relax=0.0), dict(relax=1.5), dict(max_steps=0),
                dict(max_steps=4097), dict(t_min=np.nan)):
        assert _check(raycast=bad) == E_ARG and not AR.R.check(AR.R.params(**bad)), bad
    assert _check(raycast=dict(max_steps=4096, eps=1e-5, relax=0.5, t_min=0.1, t_max=50.0)) == 0
    # sizes: rows, and the cast's tables over ALL hypotheses' rays
    three = np.stack([good] * 3)
    assert _check(T0=three, n_rays=(2 ** 31 - 1) // 3, n_obj=0) == 0 and _check(T0=three, n_rays=(2 ** 31 - 1) // 3 + 1, n_obj=0) == E_ARG
    # 64 MiB of pair counts: n_obj x ceil(rows / 64) x 4 bytes
    n_obj = 1024
    rows_ok = (64 << 20) // 4 // n_obj * 64
    assert _check(T0=three[:2], n_rays=rows_ok // 2, n_obj=n_obj) == 0 and _check(T0=three[:2], n_rays=rows_ok // 2 + 1, n_obj=n_obj) == E_ARG
    assert _check(T0=good, n_rays=rows_ok, n_obj=n_obj) == 0 and _check(T0=good, n_rays=rows_ok + 1, n_obj=n_obj) == E_ARG
    assert AR.check(dict(max_dist=0.3), {}, 1.0, 2, rows_ok // 2, n_obj) and not AR.check(dict(max_dist=0.3), {}, 1.0, 2, rows_ok // 2 + 1, n_obj)
    # 64 MiB of code biases: 16 384 objects
    assert _check(n_rays=1, n_obj=16384) == 0 and _check(n_rays=1, n_obj=16385) == E_ARG and _check(n_rays=0, n_obj=16385) == 0
    # NULL arguments
    lib = L.load()
    assert lib.dsp_debug_align_rays_check(None, None, 1.0, None, 0, None, 0, 0) == E_ARG


# ---- 3. the algorithm, float64, oracle decoder -------------------------------------------------------------------------------------------
SEED = 7
T_TRUE = A.rigid(A.axis_angle([0.3, -1.0, 0.5], 0.7), [0.5, -1.5, 2.0])


def aimed_rays(rng, t_world_obj, T_true, per_obj, spread=0.85):
    """sensor-frame unit directions from the sensor origin towards random points of a disc of radius spread x scale about every object's centre"""
    inv = np.linalg.inv(T_true)
    out = []
    for t in np.asarray(t_world_obj, F64):
        s = np.cbrt(np.linalg.det(t[:3, :3]))
        c = inv[:3, :3] @ t[:3, 3] + inv[:3, 3]
        axis = c / np.sqrt((c * c).sum())
        a = np.cross(axis, [0.0, 0.0, 1.0])
        if np.sqrt((a * a).sum()) < 1e-6:              # the object stands on the sensor's z axis
            a = np.cross(axis, [1.0, 0.0, 0.0])
        a /= np.sqrt((a * a).sum())
        b = np.cross(axis, a)
        r, phi = spread * s * np.sqrt(rng.uniform(0, 1, per_obj)), rng.uniform(0, 2 * np.pi, per_obj)
        p = c + np.outer(r * np.cos(phi), a) + np.outer(r * np.sin(phi), b)
        out.append(p / np.sqrt((p * p).sum(1))[:, None])
    return np.concatenate(out)


def _oracle_scene(dec):
    """The three-object layout of tests/test_align_host.py seen from T_TRUE by rays aimed at the objects; 16 hits per object are kept."""
    from oracle import dsp_oracle
    rng = np.random.default_rng(SEED)
    t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [2.6, 0.3, -0.2], [4.0, -3.0, 1.0]])
    codes = rng.uniform(-0.3, 0.3, (3, 64)).astype(F32)
    decode = lambda o, p: (lambda y, g, _: (y, g[:, -3:]))(*dsp_oracle._decode64(dec, codes[o].astype(F64), np.asarray(p, F64)))
    amap = A.Map(t, codes)
    dirs = aimed_rays(rng, t, T_TRUE, 40)
    pts, obj = AR.observe64(amap, decode, T_TRUE, dirs)
    keep = np.concatenate([np.flatnonzero(obj == o)[:16] for o in range(3)])
    assert keep.size == 48, [int((obj == o).sum()) for o in range(3)]
    world = pts[keep] @ T_TRUE[:3, :3].T + T_TRUE[:3, 3]
    return dict(map=amap, decode=decode, pts=pts[keep], centre=world.mean(0))


def test_algorithm_recovers_the_pose(oracle_decoder):
    s = _oracle_scene(oracle_decoder)
    rng = np.random.default_rng(SEED)
    near, mid = A.offset_pose(rng, T_TRUE, 5.0, 0.05, s["centre"]), A.offset_pose(rng, T_TRUE, 20.0, 0.2, s["centre"])
    kw = dict(max_dist=0.3, huber=0.05, trans_tol=0.0, rot_tol=0.0)
    # at the true pose the cast sees what was measured: every ray is matched.  The hit sample's own distance is anywhere in (0, eps], so a
    # residual without the first-order term would have a median near eps / 2; with it the typical residual is second order (a tenth of eps
    # is a generous bound), and the cost stays below eps^2 even with a grazing ray in the set
    ev = AR.evaluate64(T_TRUE, s["pts"], None, None, s["map"], s["decode"], 0.05, 0.3, 0.6)
    print("at the true pose: median |d| %.3e, max |d| %.3e, cost %.3e" % (np.median(np.abs(ev["dist"])), np.abs(ev["dist"]).max(), ev["cost"]))
    assert ev["n_used"] == 48 and np.median(np.abs(ev["dist"])) < 1e-4 and ev["cost"] < 1e-6, (ev["n_used"], np.abs(ev["dist"]).max(), ev["cost"])
    # The fixed point is reached by the fifth evaluation from 5 degrees (measured: 8.17e-4 / 2.05e-4 rad at every later one, and the same
    # from 20 degrees).  What is left is below the marcher's eps.  It is a property of the first-order residual on THIS decoder, not of eps
    # alone (at eps 1e-4: 7.25e-4 / 1.71e-4 rad): one ray of the 48 grazes a place where the decoder's gradient along the ray is 3.5 and
    # changes within the gap, so its d is 5e-3 at the true pose itself, and the least-squares pose gives way to it.
    for start, iters in ((near, 6), (mid, 9)):
        r = A.run(start, s["pts"], None, s["map"], s["decode"], iterations=iters, evaluate=AR.evaluator64(None, 0.6), **kw)
        et, er = A.pose_error(r["pose"], T_TRUE)
        print("ray alignment, float64, eps 1e-3: %.3e / %.3e rad after %d evaluations, %d of 48 used" % (et, er, iters, r["n_used"]))
        assert et < 1e-3 and er < 1e-3 and r["n_used"] >= 44, (et, er, r["n_used"])
        costs = [e["cost"] for e in r["trace"]]
        assert all(b <= a for a, b in zip(costs, costs[1:4])), costs          # the cost falls while the pose still moves


# ---- 4. the Python helpers on a hand-built engine ----------------------------------------------------------------------------------------
def test_localise_rays_and_depth_on_a_hand_built_result():
    seen = {}

    class Fake:
        def align_rays_to_map(self, poses, codes, pts, t0, origins=None, weights=None, trace=False, per_ray=False, **params):
            assert per_ray and poses.shape == (2, 4, 4) and len(codes) == 2
            seen.update(pts=np.asarray(pts), weights=weights, params=params, origins=origins)
            n = np.asarray(pts).reshape(-1, 3).shape[0]
            return {"obj": np.resize(np.array([0, 1, -1], np.int32), (1, n)), "dist": np.zeros((1, n), F32), "best": 0}
    objs = [dict(id=17, pose=np.eye(4), code=np.zeros(64, F32)), dict(id=4, pose=np.eye(4), code=np.zeros(64, F32))]
    res = M.localise_rays(Fake(), objs, np.zeros((3, 3)), np.eye(4), max_gap=0.7, iterations=3)
    assert res["id"].tolist() == [[17, 4, -1]] and seen["params"] == {"max_gap": 0.7, "iterations": 3} and seen["origins"] is None
    # a z-depth image: the pixel_rays convention, bad depths skipped
    K = (100.0, 120.0, 1.5, 1.0)
    depth = np.array([[2.0, np.inf, 3.0, -1.0], [0.0, 4.0, np.nan, 5.0], [1.0, 1.0, 1.0, 1.0]], F32)
    wimg = np.arange(12, dtype=F32).reshape(3, 4)
    res = M.localise_depth(Fake(), objs, depth, K, np.eye(4), weights=wimg)
    keep = [0, 2, 5, 7, 8, 9, 10, 11]
    assert res["pixel"].tolist() == keep and seen["weights"].tolist() == [float(k) for k in keep]
    _, dirs, cos = M.pixel_rays(K, np.eye(4), 4, 3)
    want = dirs.astype(F64)[keep] * depth.reshape(-1).astype(F64)[keep, None]       # z-depth x (x / z, y / z, 1)
    assert np.allclose(seen["pts"], want, rtol=1e-6, atol=0) and np.allclose(seen["pts"][:, 2], depth.reshape(-1)[keep])
