"""CPU-only: the map query (dsp_map_query, include/dsp_gn.h) above and below the device.

  * every new symbol is declared in the header, exported by the library and bound in dsp_slam_amd/_lib.py;
  * the arithmetic: dsp_debug_query_invert / _candidates / _select (csrc/query_math.h, the functions the device kernels call) against the
    numpy restatement of the same single operations in the same order (tests/query_ref.py), bit for bit -- points within a few float32 steps
    of a sphere's boundary on both sides, a NaN point and a point at an object's centre included;
  * the refused poses and the refusals that need no device;
  * map_objects.query_points / associate on a hand-built result, with no device.
"""
import os
import re

import numpy as np
import pytest

import query_ref as Q
from conftest import ROOT
from dsp_slam_amd import _lib as L
from dsp_slam_amd import map_objects as M

F32 = np.float32
NEW = ["dsp_map_query", "dsp_map_query_last_stats", "dsp_debug_query_invert", "dsp_debug_query_candidates", "dsp_debug_query_select",
       "dsp_debug_query_chunk_rows", "dsp_debug_query_plan"]
E_ARG = -1


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def host_invert(t):
    t = L.f32(t).reshape(-1, 16)
    rt, s = np.full((t.shape[0], 12), 7.0, F32), np.full(t.shape[0], 7.0, F32)
    rc = L.load().dsp_debug_query_invert(t.shape[0], L.ptr(t), L.ptr(rt), L.ptr(s))
    return rc, rt, s


def host_candidates(rt, s, pts):
    rt, s, pts = L.f32(rt).reshape(-1, 12), L.f32(s), L.f32(pts).reshape(-1, 3)
    no, npt = rt.shape[0], pts.shape[0]
    p, ins, b = np.full((no, npt, 3), 7.0, F32), np.full((no, npt), 7, np.uint8), np.full(npt, 7.0, F32)
    assert L.load().dsp_debug_query_candidates(no, L.ptr(rt), L.ptr(s), npt, L.ptr(pts), L.ptr(p), L.ptr(ins, L.C.POINTER(L.C.c_uint8)), L.ptr(b)) == 0
    return p, ins, b


def host_select(sdf, sc, ob, pt, n_pts):
    sdf, sc = L.f32(sdf), L.f32(sc)
    ob, pt = np.ascontiguousarray(ob, np.int32), np.ascontiguousarray(pt, np.int32)
    obj, dist = np.full(n_pts, 7, np.int32), np.full(n_pts, 7.0, F32)
    assert L.load().dsp_debug_query_select(sdf.shape[0], L.ptr(sdf), L.ptr(sc), L.ptr(ob, L.c_i32p), L.ptr(pt, L.c_i32p), n_pts,
                                           L.ptr(obj, L.c_i32p), L.ptr(dist)) == 0
    return obj, dist


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    assert re.search(r"#define\s+DSP_QUERY_NORMALS\s+1\b", src) and L.QUERY_NORMALS == 1
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dsp_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    bound = {n for n, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert lib.dsp_abi_version() == 6


def test_fmaf_emulation_is_one_rounding():
    """The restatement's fmaf against exact rational arithmetic, on operands built to sit on double-rounding ties and on random ones."""
    from fractions import Fraction
    rng = np.random.default_rng(20)
    a = rng.normal(size=4000).astype(F32)
    b = rng.normal(size=4000).astype(F32)
    c = (rng.normal(size=4000) * 10.0 ** rng.uniform(-9, 3, 4000)).astype(F32)
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies exactly halfway between two float32; c = +-2^-80 is lost in the float64 sum, which then rounds
    # to even either way -- one rounding of the exact value goes up for +, down for -
    a[:4] = F32(1 + 2.0 ** -12)
    b[:4] = F32(1 + 2.0 ** -12)
    c[:4] = [F32(2.0 ** -80), F32(-2.0 ** -80), F32(0), F32(2.0 ** -30)]
    got = Q.fmaf32(a, b, c)
    assert got[0] == F32(1 + 2.0 ** -11 + 2.0 ** -23) and got[1] == F32(1 + 2.0 ** -11) and got[2] == F32(1 + 2.0 ** -11)
    naive = (a[:2].astype(np.float64) * b[:2].astype(np.float64) + c[:2].astype(np.float64)).astype(F32)
    assert naive[0] != got[0]                          # the case the plain float64 emulation gets wrong
    for i in range(a.shape[0]):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F32(float(exact))                        # float(Fraction) rounds once to float64; refine against the float32 neighbours
        cands = [np.nextafter(lo, F32(-np.inf)), lo, np.nextafter(lo, F32(np.inf))]
        err = [abs(Fraction(float(x)) - exact) for x in cands]
        best = min(err)
        winners = [x for x, e in zip(cands, err) if e == best]
        if len(winners) == 2:                         # an exact tie of the float32 grid: round to even
            winners = [x for x in winners if (int(_u32(x).ravel()[0]) & 1) == 0]
        assert _u32(got[i]) == _u32(winners[0]), (i, a[i], b[i], c[i])


def _poses(rng, n, t_max=100.0):
    return Q.sim3(Q.random_rotations(rng, n), rng.uniform(0.3, 4.0, n), rng.uniform(-t_max, t_max, (n, 3)))


# ---- 1. the inversion, bit for bit ------------------------------------------------------------------------------------------------------
def test_invert_is_the_float64_restatement_bit_for_bit():
    rng = np.random.default_rng(21)
    t = _poses(rng, 64)
    rc, rt, s = host_invert(t)
    want_rt, want_s, ok = Q.invert(t)
    assert rc == 0 and ok.all()
    assert np.array_equal(_u32(rt), _u32(want_rt)) and np.array_equal(_u32(s), _u32(want_s))
    # and it IS the inverse: R_ow (s R) = I, R_ow t + t_ow = 0, to float32 accuracy
    a, tr = t[:, :3, :3].astype(np.float64), t[:, :3, 3].astype(np.float64)
    r = rt.reshape(-1, 3, 4).astype(np.float64)
    assert np.abs(r[:, :, :3] @ a - np.eye(3)).max() < 1e-6
    assert np.abs(np.einsum("nij,nj->ni", r[:, :, :3], tr) + r[:, :, 3]).max() < 1e-4
    assert np.abs(s / np.cbrt(np.linalg.det(a)) - 1).max() < 1e-6


# ---- 2. the refused poses ---------------------------------------------------------------------------------------------------------------
def test_refused_poses():
    rng = np.random.default_rng(22)
    good = _poses(rng, 1)[0]
    assert host_invert(good)[0] == 0
    sheared = good.copy()
    sheared[:3, :3] = sheared[:3, :3] @ np.array([[1, 0.01, 0], [0, 1, 0], [0, 0, 1]], F32)
    bottom = good.copy()
    bottom[3] = (0, 0, 1e-3, 1)
    bottom2 = good.copy()
    bottom2[3, 3] = 2
    nan, inf = good.copy(), good.copy()
    nan[1, 2] = np.nan
    inf[0, 3] = np.inf
    zero = good.copy()
    zero[:3, :3] = 0
    squashed = good.copy()
    squashed[:3, 0] *= 0.5                                   # anisotropic scale: not a Sim(3)
    for name, t in (("sheared", sheared), ("bottom row", bottom), ("bottom row w", bottom2), ("nan", nan), ("inf", inf), ("zero scale", zero),
                    ("anisotropic", squashed)):
        rc, rt, s = host_invert(t)
        assert rc == E_ARG and np.all(rt == 7) and np.all(s == 7), name
        assert not Q.invert(t)[2][0], name
    # one bad pose among good ones refuses the call
    many = np.stack([good, sheared, good])
    assert host_invert(many)[0] == E_ARG
    lib = L.load()
    assert lib.dsp_debug_query_invert(-1, None, None, None) == E_ARG and lib.dsp_debug_query_invert(0, None, None, None) == 0
    assert lib.dsp_debug_query_invert(1, None, None, None) == E_ARG


# ---- 3. candidates, bit for bit ---------------------------------------------------------------------------------------------------------
def _boundary_points(rt, s, t, rng, per_obj=6, reach=200):
    """World points within a few float32 steps of each object's sphere boundary, on both sides: a surface point's largest coordinate offset is stepped with nextafter
    until the reference's decision for that object flips; the points either side of the flip (and two more steps out) are returned."""
    out, sides = [], []
    for o in range(t.shape[0]):
        a, tr = t[o, :3, :3].astype(np.float64), t[o, :3, 3].astype(np.float64)
        u = rng.normal(size=(per_obj, 3))
        u /= np.sqrt((u * u).sum(1))[:, None]
        for p in (u @ a.T + tr).astype(F32):
            ax = int(np.argmax(np.abs(p.astype(np.float64) - tr)))      # the axis along which the point is farthest from the centre
            up, down = [p[ax]], [p[ax]]
            for _ in range(reach):
                up.append(np.nextafter(up[-1], F32(np.inf)))
                down.append(np.nextafter(down[-1], F32(-np.inf)))
            xs = np.array(down[::-1][:-1] + up, F32)
            line = np.tile(p, (xs.shape[0], 1))
            line[:, ax] = xs
            ins = Q.candidates(rt[o:o + 1], s[o:o + 1], line)[1][0]
            flips = np.flatnonzero(ins[1:] != ins[:-1])
            assert flips.size >= 1, "no flip within reach"
            k = flips[0]
            for j in range(max(0, k - 2), min(len(xs), k + 4)):
                out.append(line[j])
                sides.append((o, bool(ins[j])))
    return np.array(out, F32), sides


def test_candidates_are_the_float32_restatement_bit_for_bit():
    rng = np.random.default_rng(23)
    t = _poses(rng, 5, t_max=10.0)
    rt, s, ok = Q.invert(t)
    assert ok.all()
    edge, sides = _boundary_points(rt, s, t, rng)
    for o in range(5):
        assert (o, True) in sides and (o, False) in sides, o        # both sides of every object's boundary occur
    centre = t[:, :3, 3].copy()                                     # a point at each object's centre
    nanp = np.array([[0.5, np.nan, 0.25], [np.nan, np.nan, np.nan], [1.0, 2.0, np.inf]], F32)
    n_rand = 500 - edge.shape[0] - centre.shape[0] - nanp.shape[0]
    assert n_rand > 100
    pick = rng.integers(0, 5, n_rand)
    near = (np.einsum("nij,nj->ni", t[pick, :3, :3].astype(np.float64), rng.uniform(-1.2, 1.2, (n_rand, 3))) + t[pick, :3, 3]).astype(F32)
    pts = np.concatenate([edge, centre, nanp, near])
    assert pts.shape == (500, 3)
    p, ins, b = host_candidates(rt, s, pts)
    wp, wins, wb = Q.candidates(rt, s, pts)
    same = (_u32(p) == _u32(wp)) | (np.isnan(p) & np.isnan(wp))
    assert same.all()
    assert np.array_equal(ins, wins.astype(np.uint8))
    assert ((_u32(b) == _u32(wb)) | (np.isnan(b) & np.isnan(wb))).all()
    i_c, i_n = edge.shape[0], edge.shape[0] + 5
    for o in range(5):
        assert ins[o, i_c + o] == 1 and np.abs(p[o, i_c + o]).max() < 1e-5           # the centre is inside, near the origin
    assert not ins[:, i_n:i_n + 3].any() and np.isnan(b[i_n]) and np.isnan(b[i_n + 1])     # a NaN point is inside nothing, its bound is NaN
    assert 200 < ins.sum() < 2000 and np.isfinite(b[:i_n]).all()
    # no object at all: +inf; null outputs are allowed
    lib = L.load()
    b0 = np.zeros(3, F32)
    assert lib.dsp_debug_query_candidates(0, None, None, 3, L.ptr(nanp), None, None, L.ptr(b0)) == 0 and np.all(np.isposinf(b0))
    assert lib.dsp_debug_query_candidates(1, None, None, 3, L.ptr(nanp), None, None, L.ptr(b0)) == E_ARG
    assert lib.dsp_debug_query_candidates(-1, None, None, 0, None, None, None, None) == E_ARG


# ---- 4. selection -----------------------------------------------------------------------------------------------------------------------
def test_key_order_ties_and_row_order():
    vals = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 2.5, 3e38, np.inf], F32)
    o = Q.orderable(vals)
    assert np.all(np.diff(o.astype(np.int64)) > 0)                                   # monotone, -0 below +0
    assert Q.orderable(np.array([np.nan, -np.nan], F32)).tolist() == [0xffffffff, 0xffffffff] and o.max() < 0xffffffff
    # each value against each other value on one point: the smaller wins; against NaN the number wins; NaN alone is no winner
    ones = np.ones(2, F32)
    for i in range(len(vals)):
        for j in range(len(vals)):
            obj, dist = host_select([vals[i], vals[j]], ones, [0, 1], [0, 0], 1)
            k = i if i <= j else j
            assert obj[0] == (0 if i <= j else 1) and _u32(dist)[0] == _u32(vals[k]).ravel()[0], (i, j)
        obj, dist = host_select([np.nan, vals[i]], ones, [0, 1], [0, 0], 1)
        assert obj[0] == 1 and _u32(dist)[0] == _u32(vals[i]).ravel()[0]
    obj, dist = host_select([np.nan], ones[:1], [0], [0], 2)
    assert obj.tolist() == [-1, -1] and np.all(np.isposinf(dist))
    # the tie rule: equal d, the lower object index wins, in either row order; d = sdf * scale decides, not sdf
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        ob = np.array([5, 3, 9])[order]
        obj, dist = host_select(np.full(3, 0.25, F32), ones[:1].repeat(3), ob, [0, 0, 0], 1)
        assert obj[0] == 3 and dist[0] == F32(0.25)
    obj, dist = host_select([0.1, 0.05], [1.0, 4.0], [0, 1], [0, 0], 1)
    assert obj[0] == 0 and dist[0] == F32(0.1)
    # random rows, shuffled five ways: the same output, equal to the restatement
    rng = np.random.default_rng(24)
    n_rows, n_pts = 3000, 400
    sdf = (rng.normal(size=n_rows) * 0.05).astype(F32)
    sdf[rng.integers(0, n_rows, 100)] = np.nan
    sdf[::7] = np.round(sdf[::7], 2)                                                 # plenty of exact ties
    sc = rng.choice(np.array([0.5, 1.0, 2.0], F32), n_rows)
    ob = rng.integers(0, 12, n_rows).astype(np.int32)
    pt = rng.integers(0, n_pts - 20, n_rows).astype(np.int32)                        # the last 20 points have no row
    want = Q.select(sdf, sc, ob, pt, n_pts)
    assert (want[0][-20:] == -1).all() and (want[0] >= 0).sum() > 300
    for k in range(6):
        perm = np.arange(n_rows) if k == 0 else rng.permutation(n_rows)
        obj, dist = host_select(sdf[perm], sc[perm], ob[perm], pt[perm], n_pts)
        assert np.array_equal(obj, want[0]) and np.array_equal(_u32(dist), _u32(want[1])), k
    lib = L.load()
    bad_pt = np.array([n_pts], np.int32)
    o1, d1 = np.zeros(n_pts, np.int32), np.zeros(n_pts, F32)
    assert lib.dsp_debug_query_select(1, L.ptr(sdf), L.ptr(sc), L.ptr(ob, L.c_i32p), L.ptr(bad_pt, L.c_i32p), n_pts, L.ptr(o1, L.c_i32p), L.ptr(d1)) == E_ARG
    assert lib.dsp_debug_query_select(1, None, L.ptr(sc), L.ptr(ob, L.c_i32p), L.ptr(pt, L.c_i32p), n_pts, L.ptr(o1, L.c_i32p), L.ptr(d1)) == E_ARG


def test_refusals_that_need_no_device():
    lib = L.load()
    t = np.eye(4, dtype=F32).reshape(1, 16)
    c = np.zeros((1, 64), F32)
    p = np.zeros((2, 3), F32)
    o, d, b = np.zeros(2, np.int32), np.zeros(2, F32), np.zeros(2, F32)
    assert lib.dsp_map_query(None, L.ptr(t), L.ptr(c), 1, L.ptr(p), 2, 0, L.ptr(o, L.c_i32p), L.ptr(d), L.ptr(b), None) == E_ARG
    assert lib.dsp_map_query_last_stats(None, L.ptr(np.zeros(4, np.int64), L.c_i64p)) == E_ARG
    assert lib.dsp_debug_query_chunk_rows(None, 64) == E_ARG


# ---- 5. the map helpers, no device ------------------------------------------------------------------------------------------------------
def test_query_points_and_associate_on_a_hand_built_result():
    class FakeEngine(object):
        def query_map(self, t_world_obj, codes, pts_world, normals=False):
            self.args = (np.asarray(t_world_obj), [np.asarray(c) for c in codes], np.asarray(pts_world), normals)
            return {"obj": np.array([1, -1, 0, 1, 2, 0], np.int32), "dist": np.array([0.01, np.inf, -0.2, 0.5, 0.03, 0.05], F32),
                    "bound": np.array([1.0, 0.2, np.inf, 0.1, 3.0, np.nan], F32)}

    objects = [dict(id=17, pose=np.eye(4), code=np.zeros(64, F32)), dict(id=4, pose=2 * np.eye(4), code=np.ones(64, F32)),
               dict(id=0, pose=np.eye(4), code=np.zeros(64, F32))]
    eng = FakeEngine()
    pts = np.zeros((6, 3), F32)
    res = M.query_points(eng, objects, pts, normals=False)
    assert eng.args[0].shape == (3, 4, 4) and eng.args[0][1, 0, 0] == 2 and len(eng.args[1]) == 3 and eng.args[3] is False
    assert res["id"].tolist() == [4, -1, 17, 4, 0, 17] and res["obj"].tolist() == [1, -1, 0, 1, 2, 0]
    a = M.associate(res, 0.05)
    assert sorted(a) == [0, 4, 17] and a[4].tolist() == [0] and a[17].tolist() == [2, 5] and a[0].tolist() == [4]
    a = M.associate(res, 0.0)
    assert sorted(a) == [17] and a[17].tolist() == [2]
    assert M.associate(res, -1.0) == {}
    a = M.associate(res, np.inf)                                  # +inf admits every point that has an object, never the ones without
    assert sorted(a) == [0, 4, 17] and a[4].tolist() == [0, 3] and sum(len(v) for v in a.values()) == 5
    empty = M.with_ids({"obj": np.zeros(0, np.int32), "dist": np.zeros(0, F32), "bound": np.zeros(0, F32)}, [])
    assert empty["id"].shape == (0,) and M.associate(empty, 1.0) == {}
