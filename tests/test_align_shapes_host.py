"""CPU-only: shape refinement (dsp_map_align_shapes, include/dsp_gn.h) above and below the device.

  * every new symbol is declared in the header, exported by the library and bound in dsp_slam_amd/_lib.py; the ABI version stays 6;
  * dsp_debug_align_shapes_rows (the 2558 sums per object, segmented by the winner, in sequential blocks of 128 list positions) against the
    numpy restatement (tests/align_shapes_ref.py), bit for bit, at every list length around the block edges;
  * dsp_debug_align_shapes_step (the mean system, regulariser, pins, the 70-dimensional Cholesky, the trial state) against the restatement;
  * the refusals that need no device (dsp_debug_align_shapes_check);
  * the ALGORITHM in float64 (align_shapes_ref.run64 with the oracle's `complex` decoder) on three objects whose codes start at an
    unrelated draw: every object's cost falls to half or less in six evaluations;
  * map_objects.refine_shapes / refine_shapes_depth on a hand-built engine.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_ref as A
import align_rays_ref as AR
import align_shapes_ref as S
import test_align_objects_host as HO
from conftest import ROOT
from dsp_slam_amd import _lib as L
from dsp_slam_amd import map_objects as M
from test_align_rays_host import aimed_rays

F32, F64 = np.float32, np.float64
NEW = ["dsp_shapes_params_default", "dsp_map_align_shapes", "dsp_map_align_shapes_last_stats", "dsp_debug_align_shapes_rows",
       "dsp_debug_align_shapes_step", "dsp_debug_align_shapes_check"]
E_ARG = -1
HUBER, MAX_DIST = 0.05, 0.3
BLOCK = S.BLOCK


def _u64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    for name, value in (("DSP_SHAPES_CODE", "1"), ("DSP_SHAPES_POSE", "2"), ("DSP_SHAPES_DIM", "70")):
        assert re.search(r"#define %s %s\b" % (name, value), src), name
    assert "#define DSP_SHAPES_RECORD (8 + 70 * 70 + 70)" in src and "#define DSP_SHAPES_TRACE (16 + 64 + 4 + 70)" in src
    assert "Code refinement is dsp_map_align_shapes" in src and "Out of scope: scale or code refinement" not in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dsp_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    bound = {n for n, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert lib.dsp_abi_version() == 6
    assert (L.SHAPES_RECORD, L.SHAPES_TRACE, L.SHAPES_DIM, L.SHAPES_NSUM) == (8 + 4900 + 70, 154, 70, S.NSUM)
    assert lib.dsp_map_align_shapes(None, None, None, 0, None, None, None, 0, None, None, None, None, 1.0, None, None, None, None, None, None, None, None,
                                    None) == E_ARG
    assert lib.dsp_map_align_shapes_last_stats(None, None) == E_ARG
    p, sp = L.AlignParams(), L.ShapesParams()
    lib.dsp_shapes_params_default(C.byref(p), C.byref(sp))
    assert (p.iterations, p.min_points, p.max_dist, p.huber, p.damp, p.trans_tol, p.rot_tol) == (10, 6, 0.3, 0.05, 1e-4, 1e-6, 1e-6)
    assert (p.lambda0, p.up, p.down, p.lambda_min, p.lambda_max) == (0, 0, 0, 0, 0)
    assert (sp.unknowns, sp.code_reg, sp.code_anchor, sp.code_tol) == (L.SHAPES_CODE, 0.0, 0.0, 1e-6)
    lib.dsp_shapes_params_default(None, None)


# ---- 1. the segmented sums, bit for bit --------------------------------------------------------------------------------------------------
N_OBJ = 4          # object 1 gets the list length under test, object 3 never wins, objects 0 and 2 are interleaved with it


def _rows_inputs(rng, length):
    """Rows of N_OBJ objects: `length` winners for object 1, 70 for object 0, 150 for object 2 (two blocks), none for object 3, 30 rows
    without a winner; among them rows of weight 0, with a p_w, a g_w or a gcode that is not finite, and unmatched rows that still have a
    winner.  The rows are shuffled: a list is the object's rows in ascending ray order, wherever they stand."""
    winner = np.concatenate([np.full(70, 0), np.full(length, 1), np.full(150, 2), np.full(30, -1)]).astype(np.int32)
    winner = winner[rng.permutation(winner.size)]
    n = winner.size
    pw = rng.uniform(-3, 3, (n, 3)).astype(F32)
    gw = (rng.normal(size=(n, 3)) * rng.uniform(0.2, 2.0, (n, 1))).astype(F32)
    gcode = (rng.normal(size=(n, 64)) * 10.0 ** rng.uniform(-3, 0, (n, 1))).astype(F32)
    d = (rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-3, -0.3, n)).astype(F32)          # both sides of huber and of max_dist
    w = rng.uniform(0, 2, n).astype(F32)
    obj_row = winner.copy()
    special = ["unmatched", "w0", "nan_point", "inf_point", "g_nan", "g_inf", "d_inf", "d_nan", "gc_nan", "gc_inf"]
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
        elif what == "d_nan":
            d[i] = np.nan
        elif what == "gc_nan":
            gcode[i, k % 64] = np.nan
        else:
            gcode[i, (7 * k) % 64] = np.inf
    obj_row[winner < 0] = -1
    d[winner < 0] = np.inf
    return pw, winner, obj_row, d, gw, gcode, w


def host_rows(pw, winner, obj_row, d, gw, gcode, w, n_obj=N_OBJ, huber=HUBER, max_dist=MAX_DIST):
    n = pw.shape[0]
    sums = np.full((n_obj, S.NSUM), 7.0, F64)
    rc = L.load().dsp_debug_align_shapes_rows(n, L.ptr(pw), L.ptr(winner, L.c_i32p), L.ptr(obj_row, L.c_i32p), L.ptr(d), L.ptr(gw), L.ptr(gcode), L.ptr(w),
                                              n_obj, huber, max_dist, L.ptr(sums, L.c_f64p))
    return rc, sums


@pytest.mark.parametrize("length", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_segmented_sums_are_the_restatement_bit_for_bit(length):
    inp = _rows_inputs(np.random.default_rng(1200 + length), length)
    pw, winner, obj_row, d, gw, gcode, w = inp
    for weights in (w, None):
        rc, sums = host_rows(*inp[:6], weights)
        want = S.rows(*inp[:6], weights, N_OBJ, HUBER, MAX_DIST)
        assert rc == 0 and np.array_equal(_u64(sums), _u64(want)), (length, np.abs(sums - want).max())
    rc, sums = host_rows(*inp)
    assert not sums[3].any() and not np.signbit(sums[3]).any()                   # the object without a winner: +0 everywhere
    terms = S.row_terms(pw, obj_row, d, gw, gcode, w, HUBER, MAX_DIST)
    valid, used = terms[:, S.IDX_W] > 0, terms[:, S.IDX_N] == 1
    own = winner >= 0
    # a row that is not used -- a g_w or a gcode that is not finite among them -- has only its cost and its weight
    assert not terms[~used, :S.IDX_COST].any() and np.isfinite(sums).all()
    bad_gc = own & valid & (obj_row >= 0) & ~np.isfinite(gcode).all(1)
    assert bad_gc.sum() >= 3 and not used[bad_gc].any()
    k = np.flatnonzero(own & valid & (obj_row < 0))
    assert k.size >= 5 and np.all(terms[k, S.IDX_COST] == w[k].astype(F64) * (HUBER * (2 * MAX_DIST - HUBER)))
    assert sums[:, S.IDX_W].sum() == pytest.approx(terms[own, S.IDX_W].sum(), rel=1e-12) and sums[:, S.IDX_N].sum() == used[own].sum()
    assert (w[own] == 0).any() and (~np.isfinite(pw[own]).all(1)).any() and (~np.isfinite(gw[own]).all(1)).any() and used[own].sum() > 60
    assert sums[1, S.IDX_N] <= length and (length == 0) == (sums[1, S.IDX_W] == 0)


def test_pose_block_is_the_objects_system():
    """Rows whose gcode is finite: the 6 x 6 pose block and the first six of b are dsp_map_align_objects' sums of the same rows -- the same
    terms bit for bit (sign of b included), added in another order."""
    rng = np.random.default_rng(77)
    pw, winner, obj_row, d, gw, gcode, w = _rows_inputs(rng, 40)
    gcode = rng.normal(size=gcode.shape).astype(F32)
    rc, sums = host_rows(pw, winner, obj_row, d, gw, gcode, w)
    other = np.zeros((N_OBJ, A.NSUM), F64)
    assert rc == 0 and L.load().dsp_debug_align_objects_rows(pw.shape[0], L.ptr(pw), L.ptr(winner, L.c_i32p), L.ptr(obj_row, L.c_i32p), L.ptr(d), L.ptr(gw),
                                                             L.ptr(w), N_OBJ, HUBER, MAX_DIST, L.ptr(other, L.c_f64p)) == 0
    for k in range(3):
        H6, Ho = S.full_h(sums[k])[:6, :6], A.full_h(other[k])
        assert np.abs(Ho).max() > 1 and np.allclose(H6, Ho, rtol=1e-13, atol=1e-13 * np.abs(Ho).max())
        bo = other[k, A.IDX_B:A.IDX_B + 6]
        assert np.allclose(sums[k, S.IDX_B:S.IDX_B + 6], bo, rtol=1e-12, atol=1e-13 * np.abs(bo).max())
        for q in (S.IDX_COST, S.IDX_W, S.IDX_N):
            assert sums[k, q] == pytest.approx(other[k, q - S.IDX_COST + A.IDX_COST], rel=1e-13)
    term = S.row_terms(pw, obj_row, d, gw, gcode, w, HUBER, MAX_DIST)
    told = A.row_terms(pw, obj_row, d, np.where((obj_row >= 0)[:, None], gw, F32(0)), w, HUBER, MAX_DIST)
    assert np.array_equal(_u64(term[:, :6]), _u64(told[:, :6])) and np.array_equal(term[:, S.IDX_B:S.IDX_B + 6], -told[:, A.IDX_B:A.IDX_B + 6])


def test_rows_edges_and_refusals():
    inp = _rows_inputs(np.random.default_rng(5), 10)
    assert host_rows(*inp, huber=0.4, max_dist=0.3)[0] == E_ARG and host_rows(*inp, max_dist=np.inf)[0] == E_ARG
    rc, sums = host_rows(*[x[:0] for x in inp[:6]], None)
    assert rc == 0 and not sums.any()
    assert host_rows(*inp, n_obj=0)[0] == 0
    pw, winner, obj_row, d, gw, gcode, w = inp
    far = winner.copy()
    far[winner == 2] = N_OBJ + 3            # a winner index beyond the table belongs to no object
    _, a = host_rows(pw, far, obj_row, d, gw, gcode, w)
    _, b = host_rows(*inp)
    assert np.array_equal(_u64(a[[0, 1, 3]]), _u64(b[[0, 1, 3]])) and not a[2].any()
    lib = L.load()
    assert lib.dsp_debug_align_shapes_rows(1, None, None, None, None, None, None, None, 1, HUBER, MAX_DIST, L.ptr(np.zeros(S.NSUM), L.c_f64p)) == E_ARG


# ---- 2. the step -------------------------------------------------------------------------------------------------------------------------
def _system(rng, n=300):
    """H, b, W of n random rows through the host's own sums (one object)."""
    pw = rng.uniform(-2, 2, (n, 3)).astype(F32)
    gw = rng.normal(size=(n, 3)).astype(F32)
    gcode = (rng.normal(size=(n, 64)) * 0.3).astype(F32)
    d = rng.uniform(-0.2, 0.2, n).astype(F32)
    w = rng.uniform(0.1, 2, n).astype(F32)
    obj = np.zeros(n, np.int32)
    rc, sums = host_rows(pw, obj, obj, d, gw, gcode, w, n_obj=1)
    assert rc == 0 and sums[0, S.IDX_N] > 100
    return np.ascontiguousarray(S.full_h(sums[0])), np.ascontiguousarray(sums[0, S.IDX_B:S.IDX_B + 70]), float(sums[0, S.IDX_W])


def host_step(H, b, W, z, z0, code_len, unknowns, reg, anchor, damp, lam, Cm):
    sp = L.ShapesParams(unknowns, reg, anchor, 1e-6)
    st = np.full(1, -7, np.int32)
    dx, Ct, zt = np.full(70, 7.0, F64), np.full(16, 7.0, F64), np.full(64, 7.0, F64)
    rc = L.load().dsp_debug_align_shapes_step(L.ptr(np.ascontiguousarray(H, F64), L.c_f64p), L.ptr(np.ascontiguousarray(b, F64), L.c_f64p), W,
                                              L.ptr(np.ascontiguousarray(z, F64), L.c_f64p), L.ptr(np.ascontiguousarray(z0, F32)), code_len, C.byref(sp), damp,
                                              lam, L.ptr(np.ascontiguousarray(Cm, F64).reshape(-1), L.c_f64p), L.ptr(st, L.c_i32p), L.ptr(dx, L.c_f64p),
                                              L.ptr(Ct, L.c_f64p), L.ptr(zt, L.c_f64p))
    return rc, int(st[0]), dx, Ct.reshape(4, 4), zt


@pytest.mark.parametrize("unknowns", [S.U_CODE, S.U_POSE, S.U_CODE | S.U_POSE])
@pytest.mark.parametrize("code_len", [64, 32])
def test_step_is_the_restatement(unknowns, code_len):
    rng = np.random.default_rng(40 + unknowns + code_len)
    H, b, W = _system(rng)
    z0 = rng.uniform(-0.3, 0.3, 64).astype(F32)
    z0[40] = F32(-0.0)
    z = z0.astype(F64) + rng.normal(size=64) * 0.01
    z[40] = -0.0
    Cm = A.rigid(A.axis_angle([0.2, 1.0, -0.3], 0.2), [0.1, -0.2, 0.05])
    for reg, anchor, damp, lam in ((0.0, 0.0, 1e-4, 0.0), (1e-3, 0.0, 1e-4, 0.5), (0.0, 2e-2, 0.0, 1e-3), (1e-2, 1e-3, 1e-6, 0.0)):
        rc, st, dx, Ct, zt = host_step(H, b, W, z, z0, code_len, unknowns, reg, anchor, damp, lam, Cm)
        want = S.solve(H, b, W, z, z0.astype(F64), code_len, unknowns, reg, anchor, damp, lam)
        assert rc == 0 and st == L.ALIGN_OK and want is not None
        assert np.array_equal(_u64(dx), _u64(want)), np.abs(dx - want).max()
        Cw, zw = S.apply_step(want, unknowns, code_len, Cm, z)
        assert np.array_equal(_u64(zt), _u64(zw))
        assert np.all(np.abs(Ct - Cw) <= 1e-14 * np.maximum(1.0, np.abs(Cw)))
        # frozen blocks and the tail of a 32-D code: dx == 0.0 exactly, and the state's own bytes
        pins = np.array([S.pinned(i, unknowns, code_len) for i in range(70)])
        assert np.all(dx[pins] == 0.0) and np.all(dx[~pins] != 0.0)
        assert np.array_equal(_u64(zt[pins[6:]]), _u64(z[pins[6:]])) and (not pins[46] or np.signbit(zt[40]))
        if not unknowns & S.U_POSE:
            assert np.array_equal(_u64(Ct), _u64(Cm))
        # the mean system solves the same equations as numpy, to rounding
        Am = H / W
        g = b / W
        Am[6:, 6:] += (reg + anchor) * np.eye(64)
        g[6:] -= reg * z + anchor * (z - z0)
        Am += (damp + lam) * np.eye(70)
        free = np.flatnonzero(~pins)
        assert np.allclose(dx[free], np.linalg.solve(Am[np.ix_(free, free)], g[free]), rtol=1e-6, atol=1e-9)


def test_step_singular_and_refusals():
    rng = np.random.default_rng(3)
    H, b, W = _system(rng)
    z0 = rng.uniform(-0.3, 0.3, 64).astype(F32)
    z, Cm = z0.astype(F64), np.eye(4)
    both = S.U_CODE | S.U_POSE
    bad = H.copy()
    bad[10, 10] = -1.0 * W                  # an indefinite system: a pivot that is not positive
    for Hm, Wm in ((bad, W), (H, 0.0), (H, -1.0), (H, np.inf), (H * np.nan, W)):
        rc, st, dx, Ct, zt = host_step(Hm, b, Wm, z, z0, 64, both, 0.0, 0.0, 0.0, 0.0, Cm)
        assert rc == 0 and st == L.ALIGN_SINGULAR and S.solve(Hm, b, Wm, z, z0, 64, both, 0.0, 0.0, 0.0, 0.0) is None
        assert np.all(dx == 7.0) and np.all(Ct == 7.0) and np.all(zt == 7.0)                   # the outputs are untouched
    # the indefinite entry pinned away: solvable
    assert host_step(bad, b, W, z, z0, 4, both, 0.0, 0.0, 1e-4, 0.0, Cm)[1] == L.ALIGN_OK
    for kw in (dict(code_len=0), dict(code_len=65), dict(unknowns=0), dict(unknowns=4), dict(reg=-1.0), dict(anchor=np.nan)):
        a = dict(code_len=64, unknowns=both, reg=0.0, anchor=0.0)
        a.update(kw)
        assert host_step(H, b, W, z, z0, a["code_len"], a["unknowns"], a["reg"], a["anchor"], 0.0, 0.0, Cm)[0] == E_ARG, kw
    assert L.load().dsp_debug_align_shapes_step(None, None, 1.0, None, None, 64, None, 0.0, 0.0, None, None, None, None, None) == E_ARG


# ---- 3. refusals that need no device -----------------------------------------------------------------------------------------------------
def _check(w=None, n_rays=0, n_obj=3, max_gap=1.0, raycast=None, origins=True, shapes=None, **fields):
    lib = L.load()
    p, sp, rp = L.AlignParams(), L.ShapesParams(), L.RaycastParams()
    lib.dsp_shapes_params_default(C.byref(p), C.byref(sp))
    lib.dsp_raycast_params_default(C.byref(rp))
    for k, v in fields.items():
        setattr(p, k, v)
    for k, v in (shapes or {}).items():
        setattr(sp, k, v)
    for k, v in (raycast or {}).items():
        setattr(rp, k, v)
    w = None if w is None else L.f32(w)
    org = np.zeros(3, F32) if origins else None         # only tested against NULL
    return lib.dsp_debug_align_shapes_check(C.byref(p), C.byref(sp), C.byref(rp), max_gap, L.ptr(org), L.ptr(w), n_rays if w is None else w.shape[0], n_obj)


def test_every_refusal():
    assert _check() == 0 and _check(max_gap=np.inf) == 0 and _check(max_gap=0.3) == 0 and _check(n_rays=5) == 0
    # the shapes params
    for u in (1, 2, 3):
        assert _check(shapes=dict(unknowns=u)) == 0 and S.check_shapes(u, 0.0, 0.0, 1e-6)
    for u in (0, 4, 5, 8, -1):
        assert _check(shapes=dict(unknowns=u)) == E_ARG and not S.check_shapes(u, 0.0, 0.0, 1e-6), u
    for name in ("code_reg", "code_anchor", "code_tol"):
        for v in (-1e-9, np.nan, np.inf, -np.inf):
            assert _check(shapes={name: v}) == E_ARG, (name, v)
        assert _check(shapes={name: 0.0}) == 0 and _check(shapes={name: 2.5}) == 0
    # everything dsp_debug_align_objects_check refuses
    assert _check(n_rays=5, origins=False) == E_ARG and _check(n_rays=0, origins=False) == 0
    for g in (np.nan, 0.0, -1.0, float(np.nextafter(0.3, 0.0)), -np.inf):
        assert _check(max_gap=g) == E_ARG, g
    assert _check(max_dist=0.5, max_gap=0.4) == E_ARG and _check(max_dist=0.5, max_gap=0.5) == 0
    for bad in (dict(iterations=0), dict(min_points=5), dict(huber=0.4, max_dist=0.3), dict(huber=0.0), dict(max_dist=np.inf), dict(damp=-1e-9),
                dict(trans_tol=-1.0), dict(rot_tol=np.nan), dict(lambda0=1e-3), dict(lambda0=1e-3, up=4.0, down=0.5, lambda_min=1e-3, lambda_max=1e-6)):
        assert _check(max_gap=np.inf, **bad) == E_ARG, bad
    for bad in (dict(t_min=-1.0), dict(t_min=2.0, t_max=1.0), dict(eps=0.0), dict(eps=np.inf), dict(relax=0.0), dict(relax=1.5), dict(max_steps=0),
                dict(max_steps=4097), dict(t_min=np.nan)):
        assert _check(raycast=bad) == E_ARG, bad
    assert _check(raycast=dict(max_steps=4096, eps=1e-5, relax=0.5, t_min=0.1, t_max=50.0)) == 0
    for w in ([1.0, -1e-9], [np.nan], [np.inf], [-0.5, 1.0]):
        assert _check(w=w) == E_ARG
    assert _check(w=[1.0, 0.0, 2.0]) == 0
    n_obj = 1024
    rays_ok = (64 << 20) // 4 // n_obj * 64
    assert _check(n_rays=rays_ok, n_obj=n_obj) == 0 and _check(n_rays=rays_ok + 1, n_obj=n_obj) == E_ARG
    assert _check(n_rays=1, n_obj=16384) == 0 and _check(n_rays=1, n_obj=16385) == E_ARG and _check(n_rays=0, n_obj=16385) == 0
    assert _check(n_rays=2 ** 31 - 1, n_obj=0) == 0 and _check(n_rays=2 ** 31, n_obj=0) == E_ARG
    assert _check(n_obj=(1 << 18) + 1) == E_ARG
    assert L.load().dsp_debug_align_shapes_check(None, None, None, 1.0, None, None, 0, 0) == E_ARG


# ---- 4. the algorithm, float64, the oracle's `complex` decoder ----------------------------------------------------------------------------
START_SEED = 77         # the start codes: a fresh uniform(-0.3, 0.3) draw, unrelated to the true codes
AIMED = 4 * HO.PER_OBJ  # directions aimed at each object per sensor: the `complex` shapes fill less of their unit spheres than the cars


def oracle_scene(dec):
    """The layout and the sensors of tests/test_align_objects_host.py decoded with `dec`: the three objects at their TRUE poses observed in
    float64 from both sensor positions, PER_OBJ hits per object and sensor."""
    from oracle import dsp_oracle
    rng = np.random.default_rng(HO.SEED)
    t_true, codes = HO.layout(rng)

    def decode(code, p):
        y, g, _ = dsp_oracle._decode64(dec, np.asarray(code, F64)[:dec.code_len], np.asarray(p, F64))
        return y, g
    amap = A.Map(t_true, codes)
    pw, ow = [], []
    for T in HO.SENSORS:
        pts, obj = AR.observe64(amap, lambda o, p: (lambda y, g: (y, g[:, -3:]))(*decode(codes[o], p)), T, aimed_rays(rng, t_true, T, AIMED))
        keep = np.concatenate([np.flatnonzero(obj == o)[:HO.PER_OBJ] for o in range(3)])
        assert keep.size == 3 * HO.PER_OBJ, [int((obj == o).sum()) for o in range(3)]
        p, o = HO.world_rays(pts[keep], T)
        pw.append(p); ow.append(o)
    start = np.random.default_rng(START_SEED).uniform(-0.3, 0.3, (3, 64)).astype(F32)
    return dict(t_true=t_true, codes=codes, decode=decode, pts=np.concatenate(pw), org=np.concatenate(ow), start=start)


def test_algorithm_lowers_every_objects_cost(complex_decoder):
    s = oracle_scene(complex_decoder)
    res = S.run64(s["t_true"], s["start"], s["decode"], s["pts"], s["org"], iterations=6, unknowns="code", damp=1e-4, code_reg=0.0, code_anchor=0.0,
                  max_dist=MAX_DIST, huber=HUBER, trans_tol=0.0, rot_tol=0.0, code_tol=0.0)
    for k, r in enumerate(res):
        print("object %d: cost %.3e -> %.3e (ratio %.3f) after %d evaluations, %d rays used, status %d" % (
            k, r["cost0"], r["cost"], r["cost"] / r["cost0"], r["evaluations"], r["n_used"], r["status"]))
    for k, r in enumerate(res):
        assert r["cost"] <= 0.5 * r["cost0"], (k, r["cost"], r["cost0"])
        assert np.array_equal(r["correction"], np.eye(4)) and not np.array_equal(r["code"], s["start"][k].astype(F64))
    # an object that is not refined keeps its code and is never evaluated
    part = S.run64(s["t_true"], s["start"], s["decode"], s["pts"], s["org"], refine=[1, 0, 1], iterations=1, max_dist=MAX_DIST, huber=HUBER)
    assert np.array_equal(part[1]["code"], s["start"][1].astype(F64)) and part[1]["evaluations"] == 0 and part[1]["status"] == A.OK
    for k in (0, 2):
        assert part[k]["evaluations"] == 1 and part[k]["steps"] == 0 and part[k]["cost"] == res[k]["cost0"]


# ---- 5. the Python helpers on a hand-built engine ----------------------------------------------------------------------------------------
def test_refine_shapes_and_depth_on_a_hand_built_result():
    seen = {}

    class Fake:
        def align_shapes_to_rays(self, poses, codes, pts, org, weights=None, refine=None, trace=False, per_ray=False, **params):
            assert per_ray and poses.shape == (2, 4, 4) and len(codes) == 2
            seen.update(pts=np.asarray(pts), org=np.asarray(org), weights=weights, refine=refine, params=params)
            n = np.asarray(pts).reshape(-1, 3).shape[0]
            moved = np.asarray(poses, F32).copy()
            moved[0, 0, 3] += 0.5
            new = np.stack([L.code64(c) for c in codes])
            new[0, 3] = 0.25
            return {"t_world_obj": moved, "codes": new, "obj": np.resize(np.array([0, 1, -1], np.int32), n), "dist": np.zeros(n, F32)}
    objs = [dict(id=17, pose=np.eye(4), code=np.zeros(64, F32)), dict(id=4, pose=np.eye(4), code=np.ones(32, F32))]
    res, new = M.refine_shapes(Fake(), objs, np.zeros((3, 3)), np.ones((3, 3)), only=[17], unknowns="pose+code", code_reg=1e-3, iterations=3)
    assert res["id"].tolist() == [17, 4, -1] and seen["params"] == {"unknowns": "pose+code", "code_reg": 1e-3, "iterations": 3} and list(seen["refine"]) == [1, 0]
    assert [o["id"] for o in new] == [17, 4] and new[0]["pose"][0, 3] == 0.5 and new[0]["code"][3] == 0.25 and objs[0]["code"][3] == 0.0
    assert new[1]["code"].shape == (32,) and np.array_equal(new[1]["code"], objs[1]["code"]) and new[0]["code"].shape == (64,)
    with pytest.raises(ValueError):
        M.refine_shapes(Fake(), objs, np.zeros((3, 3)), np.ones((3, 3)), only=[99])
    K = (100.0, 120.0, 1.5, 1.0)
    d0 = np.array([[2.0, np.inf, 3.0, -1.0], [0.0, 4.0, np.nan, 5.0], [1.0, 1.0, 1.0, 1.0]], F32)
    d1 = np.full((3, 4), 2.0, F32)
    T1 = A.rigid(A.axis_angle([0, 1, 0], 0.3), [1.0, 2.0, 3.0])
    res, _ = M.refine_shapes_depth(Fake(), objs, [d0, d1], K, [np.eye(4), T1])
    keep = [0, 2, 5, 7, 8, 9, 10, 11]
    assert res["pixel"].tolist() == keep + list(range(12)) and res["frame"].tolist() == [0] * 8 + [1] * 12 and seen["refine"] is None
    # the rays are refine_poses_depth's
    class FakePoses:
        def align_objects_to_rays(self, poses, codes, pts, org, **kw):
            seen.update(pts2=np.asarray(pts), org2=np.asarray(org))
            n = np.asarray(pts).shape[0]
            return {"t_world_obj": np.asarray(poses, F32), "obj": np.zeros(n, np.int32), "dist": np.zeros(n, F32)}
    M.refine_poses_depth(FakePoses(), objs, [d0, d1], K, [np.eye(4), T1])
    assert np.array_equal(seen["pts"], seen["pts2"]) and np.array_equal(seen["org"], seen["org2"])
    res, _ = M.refine_shapes_depth(Fake(), objs, d0, K, np.eye(4), weights=np.arange(12, dtype=F32).reshape(3, 4))
    assert res["pixel"].tolist() == keep and seen["weights"].tolist() == [float(k) for k in keep]
