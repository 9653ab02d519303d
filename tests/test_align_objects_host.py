"""CPU-only: object refinement (dsp_map_align_objects, include/dsp_gn.h) above and below the device.

  * every new symbol is declared in the header, exported by the library and bound in dsp_slam_amd/_lib.py; the ABI version stays 6;
  * dsp_debug_align_objects_rows (the sums segmented by the winner, through align_math.h's tree over each object's list, b negated) and
    dsp_debug_align_objects_compose against the numpy restatement (tests/align_objects_ref.py), bit for bit;
  * the sign: the step of the object's system is minus the sensor's for the same rows, exactly;
  * the refusals that need no device (dsp_debug_align_objects_check);
  * the ALGORITHM in float64 (align_objects_ref.run64: float64 rays from two sensor positions, a float64 sphere tracer, the oracle's
    decoder) on three displaced objects: the condition that makes the GPU recovery test meaningful;
  * map_objects.refine_poses / refine_poses_depth on a hand-built engine.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_objects_ref as AO
import align_rays_ref as AR
import align_ref as A
import query_ref as Q
from conftest import ROOT
from dsp_slam_amd import _lib as L
from dsp_slam_amd import map_objects as M
from test_align_rays_host import aimed_rays

F32, F64 = np.float32, np.float64
NEW = ["dsp_map_align_objects", "dsp_map_align_objects_last_stats", "dsp_debug_align_objects_rows", "dsp_debug_align_objects_compose",
       "dsp_debug_align_objects_check"]
E_ARG = -1
HUBER, MAX_DIST = 0.05, 0.3


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
    assert lib.dsp_map_align_objects(None, None, None, 0, None, None, None, 0, None, None, None, 1.0, None, None, None, None, None, None, None, None) == E_ARG
    assert lib.dsp_map_align_objects_last_stats(None, None) == E_ARG


# ---- 1. the segmented sums, bit for bit --------------------------------------------------------------------------------------------------
N_OBJ = 4          # object 1 gets the list length under test, object 3 never wins, objects 0 and 2 share the rest


def _rows_inputs(rng, length):
    """Rows of N_OBJ objects: `length` winners for object 1, about 70 for object 0, about 330 for object 2 (two tree blocks), none for
    object 3, 40 rows without a winner; among them rows of weight 0, with a p_w or a g_w that is not finite, and unmatched rows that still
    have a winner.  The rows are shuffled: a list is the object's rows in ascending ray order, wherever they stand."""
    winner = np.concatenate([np.full(70, 0), np.full(length, 1), np.full(330, 2), np.full(40, -1)]).astype(np.int32)
    winner = winner[rng.permutation(winner.size)]
    n = winner.size
    pw = rng.uniform(-3, 3, (n, 3)).astype(F32)
    gw = (rng.normal(size=(n, 3)) * rng.uniform(0.2, 2.0, (n, 1))).astype(F32)
    d = (rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-3, -0.3, n)).astype(F32)          # both sides of huber and of max_dist
    w = rng.uniform(0, 2, n).astype(F32)
    obj_row = winner.copy()
    special = ["unmatched", "w0", "nan_point", "inf_point", "g_nan", "g_inf", "d_inf", "d_nan"]
    pick = rng.permutation(n)[:n // 3]
    for k, i in enumerate(pick):
        what = special[k % len(special)]
        if what == "unmatched":
            obj_row[i], d[i] = -1, (np.inf if k % 2 else d[i])
        elif what == "w0":
            w[i] = 0
        elif what == "nan_point":
            pw[i, k % 3] = np.nan
        elif what == "inf_point":
            pw[i, k % 3] = np.inf
        elif what == "g_nan":
            gw[i, k % 3] = np.nan
        elif what == "g_inf":
            gw[i, k % 3] = -np.inf
        elif what == "d_inf":
            d[i] = np.inf
        else:
            d[i] = np.nan
    obj_row[winner < 0] = -1
    d[winner < 0] = np.inf
    return pw, winner, obj_row, d, gw, w


def host_rows(pw, winner, obj_row, d, gw, w, n_obj=N_OBJ, huber=HUBER, max_dist=MAX_DIST):
    n = pw.shape[0]
    sums = np.full((n_obj, A.NSUM), 7.0, F64)
    rc = L.load().dsp_debug_align_objects_rows(n, L.ptr(pw), L.ptr(winner, L.c_i32p), L.ptr(obj_row, L.c_i32p), L.ptr(d), L.ptr(gw), L.ptr(w), n_obj, huber,
                                               max_dist, L.ptr(sums, L.c_f64p))
    return rc, sums


@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_segmented_sums_are_the_restatement_bit_for_bit(length):
    inp = _rows_inputs(np.random.default_rng(900 + length), length)
    pw, winner, obj_row, d, gw, w = inp
    for weights in (w, None):
        rc, sums = host_rows(*inp[:5], weights)
        want = AO.rows(*inp[:5], weights, N_OBJ, HUBER, MAX_DIST)
        assert rc == 0 and np.array_equal(_u64(sums), _u64(want)), (length, np.abs(sums - want).max())
    rc, sums = host_rows(*inp)
    # the object without a winner: zero sums, and the negated zero of b
    assert not sums[3].any() and np.all(np.signbit(sums[3, A.IDX_B:A.IDX_B + 6])) and not np.signbit(sums[3, :A.IDX_B]).any()
    # every object's sums are those of its own rows alone, through the plain tree (the sensor-side hook), b negated
    for k in range(N_OBJ):
        m = winner == k
        alone = np.zeros(A.NSUM, F64)
        assert L.load().dsp_debug_align_rows(int(m.sum()), L.ptr(pw[m].copy()), L.ptr(obj_row[m].copy(), L.c_i32p), L.ptr(d[m].copy()), L.ptr(gw[m].copy()),
                                             L.ptr(w[m].copy()), HUBER, MAX_DIST, L.ptr(alone, L.c_f64p)) == 0
        alone[A.IDX_B:A.IDX_B + 6] = -alone[A.IDX_B:A.IDX_B + 6]
        assert np.array_equal(_u64(sums[k]), _u64(alone)), k
    terms = A.row_terms(pw, obj_row, d, np.where((obj_row >= 0)[:, None], gw, F32(0)), w, HUBER, MAX_DIST)
    valid, used = terms[:, A.IDX_W] > 0, terms[:, A.IDX_N] == 1
    own = winner >= 0
    # unmatched rows that still have a winner cost it w rho(max_dist) and nothing else; rows without a winner are in no sum
    k = np.flatnonzero(own & valid & (obj_row < 0))
    assert k.size >= 10 and np.all(terms[k, A.IDX_COST] == w[k].astype(F64) * (HUBER * (2 * MAX_DIST - HUBER))) and not terms[k, :A.IDX_COST].any()
    assert sums[:, A.IDX_W].sum() == pytest.approx(terms[own, A.IDX_W].sum(), rel=1e-12) and sums[:, A.IDX_N].sum() == used[own].sum()
    assert (w[own] == 0).any() and (~np.isfinite(pw[own]).all(1)).any() and (~np.isfinite(gw[own]).all(1)).any() and used[own].sum() > 100
    assert sums[1, A.IDX_N] <= length and (length == 0) == (sums[1, A.IDX_W] == 0)


def test_rows_edges_and_refusals():
    inp = _rows_inputs(np.random.default_rng(5), 10)
    assert host_rows(*inp, huber=0.4, max_dist=0.3)[0] == E_ARG and host_rows(*inp, max_dist=np.inf)[0] == E_ARG
    rc, sums = host_rows(*[x[:0] for x in inp[:5]], None)
    assert rc == 0 and not sums.any()
    rc, sums = host_rows(*inp, n_obj=0)
    assert rc == 0
    # a winner index beyond the table belongs to no object
    pw, winner, obj_row, d, gw, w = inp
    far = winner.copy()
    far[winner == 2] = N_OBJ + 3
    _, a = host_rows(pw, far, obj_row, d, gw, w)
    _, b = host_rows(*inp)
    assert np.array_equal(_u64(a[[0, 1, 3]]), _u64(b[[0, 1, 3]])) and not a[2].any()


# ---- 2. the sign -------------------------------------------------------------------------------------------------------------------------
def test_the_objects_step_is_minus_the_sensors_exactly():
    rng = np.random.default_rng(31)
    n = 200
    pw = rng.uniform(-2, 2, (n, 3)).astype(F32)
    gw = rng.normal(size=(n, 3)).astype(F32)
    d = rng.uniform(-0.2, 0.2, n).astype(F32)
    w = rng.uniform(0.1, 2, n).astype(F32)
    obj = np.zeros(n, np.int32)
    lib = L.load()
    sens = np.zeros(A.NSUM, F64)
    assert lib.dsp_debug_align_rows(n, L.ptr(pw), L.ptr(obj, L.c_i32p), L.ptr(d), L.ptr(gw), L.ptr(w), HUBER, MAX_DIST, L.ptr(sens, L.c_f64p)) == 0
    rc, objs = host_rows(pw, obj, obj, d, gw, w, n_obj=1)
    assert rc == 0 and np.array_equal(_u64(objs[0, :A.IDX_B]), _u64(sens[:A.IDX_B])) and np.array_equal(_u64(objs[0, A.IDX_COST:]), _u64(sens[A.IDX_COST:]))
    steps = []
    for s in (sens, objs[0]):
        H, b = np.ascontiguousarray(A.full_h(s)), np.ascontiguousarray(s[A.IDX_B:A.IDX_B + 6])
        st, xi, tt = np.zeros(1, np.int32), np.zeros(6, F64), np.zeros(16, F64)
        assert lib.dsp_debug_align_step(L.ptr(H, L.c_f64p), L.ptr(b, L.c_f64p), 1e-9, 0.0, L.ptr(np.eye(4).reshape(-1).copy(), L.c_f64p), L.ptr(st, L.c_i32p),
                                        L.ptr(xi, L.c_f64p), L.ptr(tt, L.c_f64p)) == 0 and st[0] == L.ALIGN_OK
        steps.append(xi)
    assert np.abs(steps[0]).min() > 0 and np.array_equal(_u64(steps[1]), _u64(-steps[0])), steps


# ---- 3. compose --------------------------------------------------------------------------------------------------------------------------
def host_compose(Cs, T0):
    Cs, T0 = np.ascontiguousarray(Cs, F64).reshape(-1, 4, 4), np.ascontiguousarray(T0, F32).reshape(-1, 4, 4)
    out = np.full(T0.shape, 7.0, F32)
    assert L.load().dsp_debug_align_objects_compose(T0.shape[0], L.ptr(Cs, L.c_f64p), L.ptr(T0), L.ptr(out)) == 0
    return out


def test_compose_is_the_restatement_bit_for_bit():
    rng = np.random.default_rng(17)
    n = 64
    T0 = Q.sim3(Q.random_rotations(rng, n), rng.uniform(0.6, 1.3, n), rng.uniform(-5, 5, (n, 3)))
    T0[3, 0, 1] = F32(-0.0)                          # a negative zero survives the identity
    Cs = np.stack([A.rigid(A.axis_angle(rng.normal(size=3), rng.uniform(0, 0.5)), rng.uniform(-0.3, 0.3, 3)) for _ in range(n)])
    got = host_compose(Cs, T0)
    assert np.array_equal(_u32(got), _u32(AO.compose_all(Cs, T0)))
    assert np.allclose(got.astype(F64), Cs @ T0.astype(F64), rtol=0, atol=1e-6) and np.all(got[:, 3] == [0, 0, 0, 1])
    ident = host_compose(np.stack([np.eye(4)] * n), T0)
    assert np.array_equal(_u32(ident), _u32(T0)) and np.array_equal(_u32(AO.compose_all(np.stack([np.eye(4)] * n), T0)), _u32(T0))
    assert np.signbit(T0[3, 0, 1]) and np.signbit(ident[3, 0, 1])
    assert L.load().dsp_debug_align_objects_compose(1, None, None, None) == E_ARG and L.load().dsp_debug_align_objects_compose(0, None, None, None) == 0


# ---- 4. refusals that need no device -----------------------------------------------------------------------------------------------------
def _check(w=None, n_rays=0, n_obj=3, max_gap=1.0, raycast=None, origins=True, **fields):
    lib = L.load()
    p, rp = L.AlignParams(), L.RaycastParams()
    lib.dsp_align_params_default(C.byref(p))
    lib.dsp_raycast_params_default(C.byref(rp))
    for k, v in fields.items():
        setattr(p, k, v)
    for k, v in (raycast or {}).items():
        setattr(rp, k, v)
    w = None if w is None else L.f32(w)
    org = np.zeros(3, F32) if origins else None         # only tested against NULL
    return lib.dsp_debug_align_objects_check(C.byref(p), C.byref(rp), max_gap, L.ptr(org), L.ptr(w), n_rays if w is None else w.shape[0], n_obj)


def test_every_refusal():
    assert _check() == 0 and _check(max_gap=np.inf) == 0 and _check(max_gap=0.3) == 0 and _check(n_rays=5) == 0
    # a NULL origin array: refused as soon as there is a ray
    assert _check(n_rays=5, origins=False) == E_ARG and _check(n_rays=0, origins=False) == 0
    # what dsp_debug_align_rays_check refuses: the gate, dsp_map_align's params, dsp_map_raycast's
    for g in (np.nan, 0.0, -1.0, float(np.nextafter(0.3, 0.0)), -np.inf):
        assert _check(max_gap=g) == E_ARG, g
    assert _check(max_dist=0.5, max_gap=0.4) == E_ARG and _check(max_dist=0.5, max_gap=0.5) == 0
    for bad in (dict(iterations=0), dict(min_points=5), dict(huber=0.4, max_dist=0.3), dict(huber=0.0), dict(max_dist=np.inf), dict(damp=-1e-9),
                dict(trans_tol=-1.0), dict(rot_tol=np.nan), dict(lambda0=1e-3), dict(lambda0=1e-3, up=4.0, down=0.5, lambda_min=1e-3, lambda_max=1e-6)):
        assert _check(max_gap=np.inf, **bad) == E_ARG, bad
    for bad in (dict(t_min=-1.0), dict(t_min=2.0, t_max=1.0), dict(eps=0.0), dict(eps=np.inf), dict(relax=0.0), dict(relax=1.5), dict(max_steps=0),
                dict(max_steps=4097), dict(t_min=np.nan)):
        assert _check(raycast=bad) == E_ARG and not AO.check(dict(max_dist=0.3), bad, 1.0, True, 0, 3), bad
    assert _check(raycast=dict(max_steps=4096, eps=1e-5, relax=0.5, t_min=0.1, t_max=50.0)) == 0
    # weights
    for w in ([1.0, -1e-9], [np.nan], [np.inf], [-0.5, 1.0]):
        assert _check(w=w) == E_ARG
    assert _check(w=[1.0, 0.0, 2.0]) == 0
    # sizes beyond raycast_check_size: 64 MiB of winner counts (n_obj x ceil(n_rays / 64) x 4 bytes), 64 MiB of code biases (16 384 objects)
    n_obj = 1024
    rays_ok = (64 << 20) // 4 // n_obj * 64
    assert _check(n_rays=rays_ok, n_obj=n_obj) == 0 and _check(n_rays=rays_ok + 1, n_obj=n_obj) == E_ARG
    assert AO.check(dict(max_dist=0.3), {}, 1.0, True, rays_ok, n_obj) and not AO.check(dict(max_dist=0.3), {}, 1.0, True, rays_ok + 1, n_obj)
    assert _check(n_rays=1, n_obj=16384) == 0 and _check(n_rays=1, n_obj=16385) == E_ARG and _check(n_rays=0, n_obj=16385) == 0
    assert _check(n_rays=2 ** 31 - 1, n_obj=0) == 0 and _check(n_rays=2 ** 31, n_obj=0) == E_ARG
    assert _check(n_obj=(1 << 18) + 1) == E_ARG
    assert L.load().dsp_debug_align_objects_check(None, None, 1.0, None, None, 0, 0) == E_ARG


# ---- 5. the algorithm, float64, oracle decoder -------------------------------------------------------------------------------------------
SEED = 7
SENSORS = [A.rigid(A.axis_angle([0.3, -1.0, 0.5], 0.7), [0.5, -1.5, 2.0]), A.rigid(A.axis_angle([1.0, 0.2, -0.4], 2.1), [3.0, 2.5, -3.0])]
OFFSETS = [(5.0, 0.05), (12.0, 0.12), (20.0, 0.2)]      # per object: degrees about its own centre, translation
PER_OBJ = 50                                           # hits kept per object and sensor: 100 rays per object


def layout(rng):
    """The three objects of tests/test_align_host.py (their spheres do not overlap): TRUE poses and codes."""
    t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [2.6, 0.3, -0.2], [4.0, -3.0, 1.0]])
    return t, rng.uniform(-0.3, 0.3, (3, 64)).astype(F32)


def displaced(rng, t_true):
    """Every object moved by its own offset of OFFSETS: the poses the refinement starts from, float32."""
    return np.stack([A.offset_pose(rng, t.astype(F64), deg, tr, t[:3, 3].astype(F64)) for t, (deg, tr) in zip(t_true, OFFSETS)]).astype(F32)


def world_rays(pts_s, T):
    """sensor-frame end points of a sensor at T -> world end points and origins"""
    pts_s = np.asarray(pts_s, F64)
    return pts_s @ T[:3, :3].T + T[:3, 3], np.broadcast_to(T[:3, 3], pts_s.shape).copy()


def _oracle_scene(dec):
    from oracle import dsp_oracle
    rng = np.random.default_rng(SEED)
    t_true, codes = layout(rng)
    decode = lambda o, p: (lambda y, g, _: (y, g[:, -3:]))(*dsp_oracle._decode64(dec, codes[o].astype(F64), np.asarray(p, F64)))
    amap = A.Map(t_true, codes)
    pw, ow = [], []
    for T in SENSORS:
        pts, obj = AR.observe64(amap, decode, T, aimed_rays(rng, t_true, T, 2 * PER_OBJ))
        keep = np.concatenate([np.flatnonzero(obj == o)[:PER_OBJ] for o in range(3)])
        assert keep.size == 3 * PER_OBJ, [int((obj == o).sum()) for o in range(3)]
        p, o = world_rays(pts[keep], T)
        pw.append(p); ow.append(o)
    return dict(t_true=t_true, codes=codes, decode=decode, pts=np.concatenate(pw), org=np.concatenate(ow), t0=displaced(rng, t_true))


def test_algorithm_moves_every_object_back(oracle_decoder):
    s = _oracle_scene(oracle_decoder)
    kw = dict(max_dist=MAX_DIST, huber=HUBER, trans_tol=0.0, rot_tol=0.0)
    start = [A.pose_error(t0.astype(F64), tt.astype(F64)) for t0, tt in zip(s["t0"], s["t_true"])]
    res = AO.run64(s["t0"], s["codes"], s["decode"], s["pts"], s["org"], iterations=6, **kw)
    for k, r in enumerate(res):
        et, er = A.pose_error(r["pose"], s["t_true"][k].astype(F64))
        print("object %d: start %.3e / %.3e rad -> %.3e / %.3e rad after %d evaluations, %d rays used, status %d" % (
            k, start[k][0], start[k][1], et, er, r["evaluations"], r["n_used"], r["status"]))
        assert et <= 0.5 * start[k][0] and er <= 0.5 * start[k][1], (k, et, er, start[k])
        assert r["n_used"] >= 50
    # an object that is not refined keeps its pose and is never evaluated; it still stands in the map
    part = AO.run64(s["t0"], s["codes"], s["decode"], s["pts"], s["org"], refine=[1, 0, 1], iterations=2, **kw)
    assert np.array_equal(part[1]["correction"], np.eye(4)) and part[1]["evaluations"] == 0 and part[1]["status"] == A.OK
    assert np.array_equal(part[1]["pose"], s["t0"][1].astype(F64))
    for k in (0, 2):
        assert part[k]["evaluations"] == 2 and part[k]["steps"] == 1 and not np.array_equal(part[k]["correction"], np.eye(4))


# ---- 6. the Python helpers on a hand-built engine ----------------------------------------------------------------------------------------
def test_refine_poses_and_depth_on_a_hand_built_result():
    seen = {}

    class Fake:
        def align_objects_to_rays(self, poses, codes, pts, org, weights=None, refine=None, trace=False, per_ray=False, **params):
            assert per_ray and poses.shape == (2, 4, 4) and len(codes) == 2
            seen.update(pts=np.asarray(pts), org=np.asarray(org), weights=weights, refine=refine, params=params)
            n = np.asarray(pts).reshape(-1, 3).shape[0]
            moved = np.asarray(poses, F32).copy()
            moved[0, 0, 3] += 0.5
            return {"t_world_obj": moved, "obj": np.resize(np.array([0, 1, -1], np.int32), n), "dist": np.zeros(n, F32)}
    objs = [dict(id=17, pose=np.eye(4), code=np.zeros(64, F32)), dict(id=4, pose=np.eye(4), code=np.ones(64, F32))]
    res, new = M.refine_poses(Fake(), objs, np.zeros((3, 3)), np.ones((3, 3)), only=[17], max_gap=0.7, iterations=3)
    assert res["id"].tolist() == [17, 4, -1] and seen["params"] == {"max_gap": 0.7, "iterations": 3} and list(seen["refine"]) == [1, 0]
    assert [o["id"] for o in new] == [17, 4] and new[0]["pose"][0, 3] == 0.5 and new[1]["pose"][0, 3] == 0.0 and objs[0]["pose"][0, 3] == 0.0
    assert np.array_equal(new[1]["code"], objs[1]["code"])
    with pytest.raises(ValueError):
        M.refine_poses(Fake(), objs, np.zeros((3, 3)), np.ones((3, 3)), only=[99])
    # two z-depth frames: the pixel_rays convention, bad depths skipped, the frames concatenated
    K = (100.0, 120.0, 1.5, 1.0)
    d0 = np.array([[2.0, np.inf, 3.0, -1.0], [0.0, 4.0, np.nan, 5.0], [1.0, 1.0, 1.0, 1.0]], F32)
    d1 = np.full((3, 4), 2.0, F32)
    T1 = A.rigid(A.axis_angle([0, 1, 0], 0.3), [1.0, 2.0, 3.0])
    res, _ = M.refine_poses_depth(Fake(), objs, [d0, d1], K, [np.eye(4), T1])
    keep = [0, 2, 5, 7, 8, 9, 10, 11]
    assert res["pixel"].tolist() == keep + list(range(12)) and res["frame"].tolist() == [0] * 8 + [1] * 12 and seen["refine"] is None
    _, dirs, _ = M.pixel_rays(K, np.eye(4), 4, 3)
    want0 = dirs.astype(F64)[keep] * d0.reshape(-1).astype(F64)[keep, None]
    assert np.allclose(seen["pts"][:8], want0, rtol=1e-6, atol=0) and not seen["org"][:8].any()
    org1, dirs1, _ = M.pixel_rays(K, T1, 4, 3)
    assert np.allclose(seen["pts"][8:], org1.astype(F64) + dirs1.astype(F64) * 2.0, rtol=1e-5, atol=1e-6) and np.allclose(seen["org"][8:], org1)
    # one frame given plainly
    res, _ = M.refine_poses_depth(Fake(), objs, d0, K, np.eye(4), weights=np.arange(12, dtype=F32).reshape(3, 4))
    assert res["pixel"].tolist() == keep and seen["weights"].tolist() == [float(k) for k in keep]
