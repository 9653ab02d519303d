"""CPU-only: ray casting against the map (dsp_map_raycast, include/dsp_gn.h) above and below the device.

  * every new symbol is declared in the header, exported by the library and bound in dsp_slam_amd/_lib.py, the ABI still 6;
  * the arithmetic: dsp_debug_raycast_segments / _step (csrc/raycast_math.h, the functions the device kernels call) against the numpy
    restatement of the header's opening comment (tests/raycast_ref.py), bit for bit -- rays that miss, graze, start inside a sphere, start
    behind it and point away, void rays, clipping by t_min / t_max, every branch of the step rule;
  * every refusal of the params and the refusals that need no device;
  * map_objects.pixel_rays / render on a hand-built result, with no device.
"""
import os
import re

import numpy as np

import query_ref as Q
import raycast_ref as R
from conftest import ROOT
from dsp_slam_amd import _lib as L
from dsp_slam_amd import map_objects as M

F32 = np.float32
NEW = ["dsp_raycast_params_default", "dsp_map_raycast", "dsp_map_raycast_last_stats", "dsp_debug_raycast_check", "dsp_debug_raycast_segments",
       "dsp_debug_raycast_step"]
E_ARG = -1
U8P = L.C.POINTER(L.C.c_uint8)


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((_u32(a) == _u32(b)) | (np.isnan(a) & np.isnan(b))))


def _prm(**kw):
    p = L.RaycastParams()
    L.load().dsp_raycast_params_default(L.C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def host_segments(rt, s, org, dirs, t_min=0.0, t_max=np.inf):
    rt, s, org, dirs = L.f32(rt).reshape(-1, 12), L.f32(s), L.f32(org).reshape(-1, 3), L.f32(dirs).reshape(-1, 3)
    no, n = rt.shape[0], org.shape[0]
    void, ex = np.full(n, 7, np.uint8), np.full((no, n), 7, np.uint8)
    t0, t1 = np.full((no, n), 7.0, F32), np.full((no, n), 7.0, F32)
    oo, do = np.full((no, n, 3), 7.0, F32), np.full((no, n, 3), 7.0, F32)
    assert L.load().dsp_debug_raycast_segments(no, L.ptr(rt), L.ptr(s), n, L.ptr(org), L.ptr(dirs), t_min, t_max, L.ptr(void, U8P), L.ptr(ex, U8P),
                                               L.ptr(t0), L.ptr(t1), L.ptr(oo), L.ptr(do)) == 0
    return void.astype(bool), ex.astype(bool), t0, t1, oo, do


def host_step(t, t1, sdf, s, **kw):
    t, t1, sdf, s = L.f32(t), L.f32(t1), L.f32(sdf), L.f32(s)
    n = t.shape[0]
    dec, d, tn = np.full(n, 7, np.int32), np.full(n, 7.0, F32), np.full(n, 7.0, F32)
    p = _prm(**kw)
    assert L.load().dsp_debug_raycast_step(n, L.ptr(t), L.ptr(t1), L.ptr(sdf), L.ptr(s), L.C.byref(p), L.ptr(dec, L.c_i32p), L.ptr(d), L.ptr(tn)) == 0
    return dec, d, tn


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    assert re.search(r"#define\s+DSP_RAYCAST_NORMALS\s+1\b", src) and L.RAYCAST_NORMALS == 1
    for name, val in (("MISS", 0), ("HIT", 1), ("UNDECIDED", 2)):
        assert re.search(r"#define\s+DSP_RAYCAST_%s\s+%d\b" % (name, val), src) and getattr(L, "RAYCAST_" + name) == val == getattr(R, name)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dsp_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    bound = {n for n, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert lib.dsp_abi_version() == 6 == L.ABI_VERSION


def test_defaults_and_every_params_refusal():
    lib = L.load()
    p = _prm()
    got = dict(t_min=p.t_min, t_max=p.t_max, eps=p.eps, relax=p.relax, max_steps=p.max_steps)
    assert got == {k: (F32(v) if k != "max_steps" else v) for k, v in R.DEFAULTS.items()}
    hdr = open(os.path.join(ROOT, "dsp_slam_amd", "csrc", "raycast_math.h")).read()
    assert "t_min 0, t_max +inf, eps 1e-3, relax 1, max_steps 64" in hdr
    assert lib.dsp_debug_raycast_check(L.C.byref(p)) == 0 and R.check(R.params())
    assert lib.dsp_debug_raycast_check(None) == E_ARG
    bad = [dict(t_min=-1e-6), dict(t_min=np.nan), dict(t_min=np.inf), dict(t_max=0.0), dict(t_min=2.0, t_max=2.0), dict(t_max=np.nan),
           dict(eps=0.0), dict(eps=-1.0), dict(eps=np.inf), dict(eps=np.nan), dict(relax=0.0), dict(relax=1.0001), dict(relax=np.nan),
           dict(relax=-0.5), dict(max_steps=0), dict(max_steps=4097), dict(max_steps=-3)]
    for kw in bad:
        assert lib.dsp_debug_raycast_check(L.C.byref(_prm(**kw))) == E_ARG, kw
        assert not R.check(R.params(**kw)), kw
    good = [dict(t_min=0.0, t_max=1e-30), dict(t_max=np.inf), dict(t_min=5.0, t_max=5.5), dict(eps=1e-30), dict(relax=1.0), dict(relax=1e-3),
            dict(max_steps=1), dict(max_steps=4096)]
    for kw in good:
        assert lib.dsp_debug_raycast_check(L.C.byref(_prm(**kw))) == 0, kw
        assert R.check(R.params(**kw)), kw
    # the step hook refuses bad params too
    one = np.zeros(1, F32)
    i1 = np.zeros(1, np.int32)
    assert lib.dsp_debug_raycast_step(1, L.ptr(one), L.ptr(one), L.ptr(one), L.ptr(one), L.C.byref(_prm(eps=0.0)), L.ptr(i1, L.c_i32p), L.ptr(one),
                                      L.ptr(one)) == E_ARG
    assert lib.dsp_debug_raycast_step(1, None, L.ptr(one), L.ptr(one), L.ptr(one), L.C.byref(_prm()), L.ptr(i1, L.c_i32p), L.ptr(one), L.ptr(one)) == E_ARG


def _scene(rng, n_obj=6):
    return Q.sim3(Q.random_rotations(rng, n_obj), rng.uniform(0.3, 4.0, n_obj), rng.uniform(-10, 10, (n_obj, 3)))


def _rays(rng, t, per_obj=60):
    """Rays of every kind about every object: through it from outside, grazing (closest approach within a few 1e-7 of the sphere's radius, on
    both sides), starting inside, starting behind it and pointing away, far misses; directions of any length."""
    org, dirs, kind = [], [], []
    for o in range(t.shape[0]):
        a, c = t[o, :3, :3].astype(np.float64), t[o, :3, 3].astype(np.float64)
        s = np.cbrt(np.linalg.det(a))
        for k in range(per_obj):
            v = rng.normal(size=3)
            v /= np.linalg.norm(v)
            w = np.cross(v, rng.normal(size=3))
            w /= np.linalg.norm(w)
            what = k % 5
            if what == 0:       # through: closest approach inside the sphere
                start, d = c + s * (rng.uniform(0, 0.9) * w - 3.0 * v), v
            elif what == 1:     # grazing
                start, d = c + s * ((1.0 + rng.choice([-3e-7, -1e-7, 0.0, 1e-7, 3e-7])) * w - 2.0 * v), v
            elif what == 2:     # starts inside
                start, d = c + s * rng.uniform(0, 0.95) * w, v
            elif what == 3:     # the sphere lies behind the origin
                start, d = c + s * (0.3 * w + 2.0 * v), v
            else:               # far miss
                start, d = c + s * (2.5 * w - 3.0 * v), v
            org.append(start)
            dirs.append(d * 10.0 ** rng.uniform(-3, 3))
            kind.append(what)
    return np.array(org, F32), np.array(dirs, F32), np.array(kind)


def test_segments_are_the_restatement_bit_for_bit():
    rng = np.random.default_rng(60)
    t = _scene(rng)
    rt, s, ok = Q.invert(t)
    assert ok.all()
    org, dirs, kind = _rays(rng, t)
    # void rays: NaN, inf, a zero direction, a direction whose squared length overflows; and an object that is never hit (NaN scale)
    void_rows = [((np.nan, 0, 0), (0, 0, 1)), ((0, 0, 0), (0, np.nan, 1)), ((np.inf, 0, 0), (0, 0, 1)), ((0, 0, 0), (1, -np.inf, 0)),
                 ((1, 2, 3), (0, 0, 0)), ((1, 2, 3), (-0.0, 0.0, 0.0)), ((0, 0, 0), (3e19, 3e19, 3e19)), ((0, 0, 0), (1e-30, 0, 0))]
    org = np.concatenate([org, np.array([v[0] for v in void_rows], F32)])
    dirs = np.concatenate([dirs, np.array([v[1] for v in void_rows], F32)])
    s_sel = s.copy()
    s_sel[4] = np.nan
    for t_min, t_max in ((0.0, np.inf), (0.5, 6.0), (2.0, 2.5)):
        void, ex, t0, t1, oo, do = host_segments(rt, s_sel, org, dirs, t_min, t_max)
        u, wvoid = R.rays(org, dirs)
        w = R.segments(rt, s_sel, org, u, wvoid, t_min, t_max)
        assert np.array_equal(void, wvoid) and wvoid[-8:].all() and not wvoid[:-8].any()
        assert np.array_equal(ex, w["exists"])
        live = ~wvoid
        for got, want in ((t0, w["t0"]), (t1, w["t1"]), (oo, w["o_o"]), (do, w["d_o"])):
            assert _same_bits(got[:, live], want[:, live])
            assert np.all(got[:, wvoid] == 0)                       # the pairs of a void ray read 0
        assert not ex[4].any() and not ex[:, wvoid].any()
        if t_min == 0.0 and t_max == np.inf:
            n = kind.size
            own = ex[np.repeat(np.arange(t.shape[0]), n // t.shape[0]), np.arange(n)]
            assert own[(kind == 0) & (np.arange(n) // 60 != 4)].all() and own[(kind == 2) & (np.arange(n) // 60 != 4)].all()
            assert not own[kind == 3].any() and not own[kind == 4].any()
            graze = own[(kind == 1) & (np.arange(n) // 60 != 4)]
            assert 0 < graze.sum() < graze.size                     # grazing rays fall on both sides of disc > 0
            inside = (kind == 2) & (np.arange(n) // 60 != 4)
            rows = np.repeat(np.arange(t.shape[0]), n // t.shape[0])[inside]
            assert np.all(t0[rows, np.flatnonzero(inside)] == 0)    # a ray that starts inside starts its march at t_min
        else:
            e = ex
            assert np.all(t0[e] >= F32(t_min)) and np.all(t1[e] <= F32(t_max)) and (t0[e] == F32(t_min)).any() and (t1[e] == F32(t_max)).any()
        # the unit direction scales nothing: |d_o| = 1 / s to float32 accuracy
        assert np.abs(np.sqrt((do[:, live].astype(np.float64) ** 2).sum(2)) * s[:, None] - 1).max() < 1e-5
    lib = L.load()
    assert lib.dsp_debug_raycast_segments(-1, None, None, 0, None, None, 0.0, 1.0, None, None, None, None, None, None) == E_ARG
    assert lib.dsp_debug_raycast_segments(1, None, None, 0, None, None, 0.0, 1.0, None, None, None, None, None, None) == E_ARG
    assert lib.dsp_debug_raycast_segments(0, None, None, 1, None, None, 0.0, 1.0, None, None, None, None, None, None) == E_ARG
    assert lib.dsp_debug_raycast_segments(0, None, None, 0, None, None, 0.0, 1.0, None, None, None, None, None, None) == 0


def test_every_branch_of_the_step_rule():
    eps, relax = F32(1e-3), F32(0.75)
    # hand-built: dist == eps hits; the next float above advances; NaN misses; t' == t1 advances, the next float below t1 as the bound exits
    t = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 0.5, 3.0, 1.0, 1.0], F32)
    sdf = np.array([1e-3, np.nextafter(F32(1e-3), F32(1)), np.nan, -0.2, 0.4, 0.4, np.inf, -np.inf, 0.0, -0.0], F32)
    s = np.ones(10, F32)
    t1 = np.full(10, 9.0, F32)
    tn4 = Q.fmaf32(relax, F32(0.4), F32(1.0))
    t1[4] = tn4                                             # t' == t1: advance
    t1[5] = np.nextafter(Q.fmaf32(relax, F32(0.4), F32(2.0)), F32(0))      # t' just above t1: exit
    dec, d, tn = host_step(t, t1, sdf, s, eps=float(eps), relax=float(relax))
    assert dec.tolist() == [R.STEP_HIT, R.STEP_ADVANCE, R.STEP_MISS, R.STEP_HIT, R.STEP_ADVANCE, R.STEP_EXIT, R.STEP_EXIT, R.STEP_HIT, R.STEP_HIT,
                            R.STEP_HIT]
    assert tn[0] == t[0] and tn[4] == tn4 and tn[2] == t[2] and np.isposinf(tn[6]) and np.isneginf(d[7])
    # dist is sdf * s: the scale decides
    dec2, d2, _ = host_step([1.0, 1.0], [9.0, 9.0], [4e-4, 4e-4], [2.0, 4.0], eps=1e-3, relax=1.0)
    assert dec2.tolist() == [R.STEP_HIT, R.STEP_ADVANCE] and d2[1] == F32(4e-4) * F32(4)
    # random, against the restatement, bit for bit
    rng = np.random.default_rng(61)
    n = 5000
    t = rng.uniform(0, 50, n).astype(F32)
    sdf = (rng.normal(size=n) * 0.05).astype(F32)
    sdf[rng.integers(0, n, 60)] = np.nan
    sdf[rng.integers(0, n, 60)] = F32(1e-3)
    s = rng.choice(np.array([0.5, 1.0, 3.0], F32), n)
    t1 = (t + rng.uniform(0, 0.1, n)).astype(F32)
    for eps_, relax_ in ((1e-3, 1.0), (1e-3, 0.5), (5e-3, 0.9)):
        dec, d, tn = host_step(t, t1, sdf, s, eps=eps_, relax=relax_)
        wdec, wd, wtn = R.step(t, t1, sdf, s, eps_, relax_)
        assert np.array_equal(dec, wdec) and _same_bits(d, wd) and _same_bits(tn, wtn)
        assert set(np.unique(dec)) == {0, 1, 2, 3}


def test_refusals_that_need_no_device():
    lib = L.load()
    t = np.eye(4, dtype=F32).reshape(1, 16)
    c = np.zeros((1, 64), F32)
    o, d = np.zeros((2, 3), F32), np.ones((2, 3), F32)
    ob, st, tt, dd = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, F32), np.zeros(2, F32)
    p = _prm()
    assert lib.dsp_map_raycast(None, L.ptr(t), L.ptr(c), 1, L.ptr(o), L.ptr(d), 2, L.C.byref(p), 0, L.ptr(ob, L.c_i32p), L.ptr(tt), L.ptr(dd),
                               L.ptr(st, L.c_i32p), None) == E_ARG
    assert lib.dsp_map_raycast_last_stats(None, L.ptr(np.zeros(6, np.int64), L.c_i64p)) == E_ARG
    lib.dsp_raycast_params_default(None)                    # a null pointer is ignored


def test_pixel_rays_and_render_on_a_hand_built_result():
    K = np.array([[100.0, 0, 3.0], [0, 50.0, 2.0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Q.random_rotations(np.random.default_rng(62), 1)[0]
    T[:3, 3] = (1.0, -2.0, 0.5)
    org, dirs, cos = M.pixel_rays(K, T, 6, 4)
    assert org.shape == dirs.shape == (24, 3) and org.dtype == dirs.dtype == F32 and np.all(org == T[:3, 3].astype(F32))
    # the principal point's pixel looks along the optical axis; row-major order: index = row * width + column
    k = 2 * 6 + 3
    assert np.allclose(dirs[k], T[:3, 2], atol=1e-6) and abs(cos[k] - 1) < 1e-6
    d_cam = dirs.astype(np.float64) @ T[:3, :3]
    assert np.allclose(d_cam[1], [(1 - 3.0) / 100, (0 - 2.0) / 50, 1], atol=1e-6) and np.allclose(d_cam[6], [(0 - 3.0) / 100, (1 - 2.0) / 50, 1], atol=1e-6)
    org2, dirs2, _ = M.pixel_rays((100.0, 50.0, 3.0, 2.0), T, 6, 4)
    assert np.array_equal(dirs, dirs2)

    class FakeEngine(object):
        def cast_rays(self, t_world_obj, codes, origins, dirs, normals=False, **params):
            self.args = (np.asarray(t_world_obj), len(codes), np.asarray(origins), np.asarray(dirs), normals, params)
            n = origins.shape[0]
            obj = np.where(np.arange(n) % 3 == 0, -1, np.arange(n) % 2).astype(np.int32)
            t = np.where(obj >= 0, 2.0 + np.arange(n), np.inf).astype(F32)
            return {"obj": obj, "t": t, "dist": np.where(obj >= 0, 1e-4, np.inf).astype(F32), "status": (obj >= 0).astype(np.int32),
                    "normal": np.ones((n, 3), F32) if normals else None}

    objects = [dict(id=17, pose=np.eye(4), code=np.zeros(64, F32)), dict(id=4, pose=2 * np.eye(4), code=np.ones(64, F32))]
    eng = FakeEngine()
    img = M.render(eng, objects, K, T, 6, 4, normals=True, eps=2e-3)
    assert eng.args[1] == 2 and eng.args[4] is True and eng.args[5] == {"eps": 2e-3} and np.array_equal(eng.args[3], dirs)
    assert img["depth"].shape == img["id"].shape == img["status"].shape == (4, 6) and img["normal"].shape == (4, 6, 3)
    flat_obj = img["obj"].reshape(-1)
    assert np.array_equal(img["id"].reshape(-1), np.where(flat_obj < 0, -1, np.where(flat_obj == 0, 17, 4)))
    hit = flat_obj >= 0
    assert np.all(np.isposinf(img["depth"].reshape(-1)[~hit]))
    assert np.allclose(img["depth"].reshape(-1)[hit], (img["t"].reshape(-1)[hit].astype(np.float64) * cos[hit]).astype(F32), rtol=0, atol=0)
    res = M.cast_rays(eng, objects, org, dirs)
    assert res["id"].tolist() == img["id"].reshape(-1).tolist() and res["normal"] is None
