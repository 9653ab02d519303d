"""GPU: the map query (include/dsp_gn.h dsp_map_query): signed distance and normal of world points to a map of posed objects.

The expected values are composed from entry points that existed before it (query_ref.expected): tests/query_ref.py for transforms,
containment and bounds (pinned on the CPU by tests/test_query_host.py), Engine.decode_sdf / Engine.sdf_jacobian per object at the
reference's object-frame points, query_ref for selection and normals.  Comparisons are bit for bit: the decoder forms are bit-identical
across tile lists by the suite's own assertions (tests/test_gpu_surface.py, tests/test_gpu_decoders.py), so no tolerance is needed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import query_ref as Q
from conftest import ROOT
from dsp_slam_amd import engine as E, _lib as L
from dsp_slam_amd import map_objects as M

pytestmark = pytest.mark.gpu

F32 = np.float32
ULP1 = 2.0 ** -23           # spacing of float32 at 1


def _engine(dec):
    return E.Engine(dec.layers, dec.latent_in, dec.code_len, device=0)


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = _engine(oracle_decoder)
    yield e
    e.close()


def _codes(seed, n, code_len=64):
    return list(np.random.default_rng(seed).uniform(-0.3, 0.3, (n, code_len)).astype(F32))


def _u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((_u32(a) == _u32(b)) | (np.isnan(a) & np.isnan(b))))


def _same(got, want, keys=("obj", "dist", "bound")):
    for k in keys:
        if k == "obj":
            assert np.array_equal(got[k], want[k]), k
        else:
            assert _bits_equal(got[k], want[k]), k


def _in_ball(rng, n, r=1.0):
    u = rng.normal(size=(n, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    return u * (r * rng.uniform(0, 1, (n, 1)) ** (1 / 3))


def _world(t, p_obj):
    return (p_obj @ t[:3, :3].astype(np.float64).T + t[:3, 3].astype(np.float64)).astype(F32)


# ---- the scene of tests 2, 5, 6, 7: three objects, two of the spheres overlapping ---------------------------------------------------------
_SCENE = {}


def scene3(eng):
    """Poses, codes, 300 points (at least 40 in the overlap of spheres 0 and 1) and the expected result with normals; computed once, never modified."""
    if not _SCENE:
        rng = np.random.default_rng(41)
        t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [1.25, 0.3, -0.2], [4.0, -3.0, 1.0]])
        codes = _codes(42, 3)
        lens = []
        while sum(len(x) for x in lens) < 120:           # points of sphere 0 that the reference also puts inside sphere 1
            cand = _world(t[0], _in_ball(rng, 400))
            ins = Q.candidates(*Q.invert(t)[:2], cand)[1]
            lens.append(cand[ins[0] & ins[1]])
        lens = np.concatenate(lens)[:120]
        inside = np.concatenate([_world(t[o], _in_ball(rng, 35, 0.98)) for o in range(3)])
        outside = np.concatenate([_world(t[o], _in_ball(rng, 25, 1.0) * 1.7) for o in range(3)])
        pts = np.concatenate([lens, inside, outside])
        assert pts.shape == (300, 3)
        _SCENE.update(t=t, codes=codes, pts=pts, exp=Q.expected(eng, t, codes, pts, with_normals=True))
        ins = _SCENE["exp"]["inside"]
        assert (ins[0] & ins[1]).sum() >= 40 and (~ins.any(0)).sum() >= 20
    return _SCENE


# ---- 1. one object, identity pose --------------------------------------------------------------------------------------------------------
def test_one_object_identity_pose(eng):
    rng = np.random.default_rng(43)
    code = _codes(44, 1)[0]
    pts = np.concatenate([_in_ball(rng, 100, 0.99), _in_ball(rng, 100) * 0.5 + np.sign(rng.normal(size=(100, 3))) * 0.9]).astype(F32)
    t = np.eye(4, dtype=F32)[None]
    exp = Q.expected(eng, t, [code], pts)
    n_in = int(exp["inside"][0].sum())
    assert 90 <= n_in <= 110                               # half outside the sphere
    res = eng.query_map(t, [code], pts)
    _same(res, exp)
    assert set(np.unique(res["obj"])) == {-1, 0} and (res["obj"] == 0).sum() == n_in
    # with the identity pose p_o is p_w: dist is decode_sdf at the points themselves, bit for bit, and the bound is |p| - 1
    idx = np.flatnonzero(exp["inside"][0])
    assert _bits_equal(exp["p_obj"][0], pts) and _bits_equal(res["dist"][idx], eng.decode_sdf(code, pts[idx]))
    out = np.flatnonzero(~exp["inside"][0])
    assert np.all(np.isposinf(res["dist"][out])) and np.all(np.isposinf(res["bound"][idx]))
    assert np.allclose(res["bound"][out], np.sqrt((pts[out].astype(np.float64) ** 2).sum(1)) - 1, atol=1e-6)
    assert eng.query_stats() == {"rows": n_in, "tiles": (n_in + 63) // 64, "chunks": 1, "passes": 1}


# ---- 2. three objects, overlapping spheres -----------------------------------------------------------------------------------------------
def test_three_objects_with_overlapping_spheres(eng):
    s = scene3(eng)
    res = eng.query_map(s["t"], s["codes"], s["pts"])
    _same(res, s["exp"])
    ins = s["exp"]["inside"]
    both = ins[0] & ins[1]
    assert set(np.unique(res["obj"][both])) == {0, 1}      # the overlap is decided by distance, both ways
    assert eng.query_stats()["rows"] == int(ins.sum())


# ---- 3. the same object listed twice -----------------------------------------------------------------------------------------------------
def test_the_same_object_twice_reports_the_lower_index(eng):
    s = scene3(eng)
    t = np.stack([s["t"][2], s["t"][1], s["t"][1], s["t"][2]])
    codes = [s["codes"][2], s["codes"][1], s["codes"][1], s["codes"][2]]
    res = eng.query_map(t, codes, s["pts"])
    alone = eng.query_map(t[:2], codes[:2], s["pts"])
    assert np.array_equal(res["obj"], alone["obj"]) and _bits_equal(res["dist"], alone["dist"])
    assert set(np.unique(res["obj"])) == {-1, 0, 1} and (res["obj"] >= 0).sum() > 100
    _same(res, Q.expected(eng, t, codes, s["pts"]))


# ---- 4. tile raggedness ------------------------------------------------------------------------------------------------------------------
def test_ragged_tiles(eng):
    rng = np.random.default_rng(45)
    want = [0, 1, 63, 64, 65]
    t = Q.sim3(Q.random_rotations(rng, 5), [0.5, 1.0, 2.0, 0.7, 1.4], [[10.0 * o, 3.0 * (o % 2), -2.0 * o] for o in range(5)])
    rt, sc, ok = Q.invert(t)
    parts = [_world(t[0], _in_ball(rng, 30) * 0.5 + 1.3)]          # 30 points near object 0 but outside it, and outside everything
    for o, n in enumerate(want):
        got = np.zeros((0, 3), F32)
        while got.shape[0] < n:                                   # rejection against the reference's containment
            cand = _world(t[o], _in_ball(rng, 2 * n + 8, 0.999))
            got = np.concatenate([got, cand[Q.candidates(rt[o:o + 1], sc[o:o + 1], cand)[1][0]]])
        parts.append(got[:n])
    pts = np.concatenate(parts)[rng.permutation(30 + sum(want))]
    codes = _codes(46, 5)
    exp = Q.expected(eng, t, codes, pts)
    assert exp["inside"].sum(1).tolist() == want and (exp["inside"].sum(0) <= 1).all()
    res = eng.query_map(t, codes, pts)
    _same(res, exp)
    # tiles hold up to 64 rows of ONE object: ceil(1/64) + ceil(63/64) + ceil(64/64) + ceil(65/64) = 1 + 1 + 1 + 2
    assert eng.query_stats() == {"rows": 193, "tiles": 5, "chunks": 1, "passes": 1}


# ---- 5. chunking -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [64, 100])
def test_chunked_runs_are_the_unchunked_run(eng, rows):
    s = scene3(eng)
    lib = L.load()
    whole = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    n_rows = eng.query_stats()["rows"]
    assert lib.dsp_debug_query_chunk_rows(eng._h, rows) == 0
    try:
        chunked = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
        st = eng.query_stats()
        plain = eng.query_map(s["t"], s["codes"], s["pts"])
    finally:
        assert lib.dsp_debug_query_chunk_rows(eng._h, 0) == 0
    _same(chunked, whole, keys=("obj", "dist", "bound", "normal"))
    _same(plain, whole)
    # a chunk ends inside an object's rows, and a chunk holds rows of several objects: the chunk borders and the object borders differ
    cnt = s["exp"]["inside"].sum(1)
    chunk_ends, obj_ends = set(range(rows, n_rows, rows)), set(np.cumsum(cnt)[:-1].tolist())
    assert st["rows"] == n_rows == cnt.sum() and st["chunks"] == -(-n_rows // rows) > 1
    assert chunk_ends - obj_ends and obj_ends - chunk_ends
    assert lib.dsp_debug_query_chunk_rows(eng._h, -1) == -1 and lib.dsp_debug_query_chunk_rows(eng._h, (1 << 24) + 1) == -1


# ---- 6. normals --------------------------------------------------------------------------------------------------------------------------
def test_normals(eng):
    s = scene3(eng)
    exp = s["exp"]
    res = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    _same(res, exp, keys=("obj", "dist", "bound", "normal"))
    _same(res, eng.query_map(s["t"], s["codes"], s["pts"]))                        # the flag changes no bit of obj, dist or bound
    hit = res["obj"] >= 0
    length = np.sqrt((res["normal"][hit].astype(np.float64) ** 2).sum(1))
    assert hit.sum() > 150 and np.abs(length - 1).max() <= 2 * ULP1
    assert np.all(res["normal"][~hit] == 0) and (~hit).sum() >= 20
    # sanity, not parity: central differences of dist along the world axes (step 1e-3 x scale) point the same way to within 5 degrees, for
    # points with |dist| < 0.05 s.  dist is the minimum over objects, so a point qualifies only where all six neighbours have its winner.
    scale = exp["scale"][np.maximum(res["obj"], 0)]
    near = np.flatnonzero(hit & (np.abs(res["dist"]) < 0.05 * scale))
    assert near.size >= 10
    h = (1e-3 * scale[near]).astype(F32)
    grad = np.zeros((near.size, 3))
    same_winner = np.ones(near.size, bool)
    for k in range(3):
        d = []
        for sign in (1, -1):
            p = s["pts"][near].copy()
            p[:, k] += sign * h
            r = eng.query_map(s["t"], s["codes"], p)
            same_winner &= r["obj"] == res["obj"][near]
            d.append((r["dist"].astype(np.float64), p[:, k].astype(np.float64)))
        with np.errstate(invalid="ignore"):
            grad[:, k] = (d[0][0] - d[1][0]) / (d[0][1] - d[1][1])
    assert same_winner.sum() >= 10
    g = grad[same_winner]
    cos = (g * res["normal"][near][same_winner]).sum(1) / np.sqrt((g * g).sum(1))
    print("central differences: %d points, worst angle %.3f deg" % (g.shape[0], np.degrees(np.arccos(np.clip(cos.min(), -1, 1)))))
    assert cos.min() >= np.cos(np.radians(5.0))


# ---- 7. determinism and equivariance -----------------------------------------------------------------------------------------------------
def test_determinism_and_equivariance(eng):
    s = scene3(eng)
    a = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    b = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    for k in ("obj", "dist", "bound", "normal"):
        assert a[k].tobytes() == b[k].tobytes(), k
    rng = np.random.default_rng(47)
    perm = rng.permutation(300)
    c = eng.query_map(s["t"], s["codes"], s["pts"][perm], normals=True)
    for k in ("obj", "dist", "bound", "normal"):
        assert c[k].tobytes() == a[k][perm].tobytes(), k
    # no exact ties between objects on this input (asserted on the reference's rows), so the winner does not depend on the object order
    rows = s["exp"]["rows"]
    d = rows["sdf"] * rows["scale"]
    for p in np.flatnonzero(s["exp"]["inside"].sum(0) > 1):
        dp = d[rows["pt"] == p]
        assert np.unique(dp).size == dp.size
    for order in ([2, 0, 1], [1, 2, 0], [2, 1, 0]):
        r = eng.query_map(s["t"][order], [s["codes"][o] for o in order], s["pts"], normals=True)
        new_index = np.argsort(order)                       # object o of the original map is object new_index[o] of the permuted one
        assert np.array_equal(r["obj"], np.where(a["obj"] >= 0, new_index[np.maximum(a["obj"], 0)], -1))
        assert _bits_equal(r["dist"], a["dist"]) and _bits_equal(r["bound"], a["bound"]) and _bits_equal(r["normal"], a["normal"])


def test_more_points_than_one_pass(eng):
    """131 072 points are one pass: 131 072 + 129 points cross the pass boundary with a 129-point tail (three waves, the last with one point)."""
    rng = np.random.default_rng(48)
    n = (1 << 17) + 129
    t = Q.sim3(Q.random_rotations(rng, 2), [0.9, 1.1], [[0.0, 0.0, 0.0], [60.0, 0.0, 0.0]])
    pts = rng.uniform(-30, 90, (n, 3)).astype(F32) * np.array([1, 0.05, 0.05], F32)      # a thin cloud along x: a few hundred points inside
    pts[-129:] = _world(t[1], _in_ball(rng, 129, 0.9))                                  # the tail lies inside object 1
    pts[(1 << 17) - 40:(1 << 17)] = _world(t[0], _in_ball(rng, 40, 0.9))                # the end of pass 0 inside object 0
    codes = _codes(49, 2)
    exp = Q.expected(eng, t, codes, pts)
    assert 169 <= exp["inside"].sum() < 20000
    res = eng.query_map(t, codes, pts, normals=True)
    _same(res, exp)
    st = eng.query_stats()
    assert st["passes"] == 2 and st["rows"] == int(exp["inside"].sum()) and (res["obj"][-129:] == 1).all()


# ---- 8. edges ----------------------------------------------------------------------------------------------------------------------------
def test_empty_map_and_no_points(eng):
    s = scene3(eng)
    r = eng.query_map(np.zeros((0, 4, 4), F32), [], s["pts"][:7], normals=True)
    assert np.all(r["obj"] == -1) and np.all(np.isposinf(r["dist"])) and np.all(np.isposinf(r["bound"])) and np.all(r["normal"] == 0)
    assert eng.query_stats() == {"rows": 0, "tiles": 0, "chunks": 0, "passes": 0}
    r = eng.query_map(s["t"], s["codes"], np.zeros((0, 3), F32), normals=True)
    assert r["obj"].shape == (0,) and r["normal"].shape == (0, 3)
    lib = L.load()
    assert lib.dsp_map_query(eng._h, None, None, 0, None, 0, 0, None, None, None, None) == 0
    # points far from everything: no candidate row, no decoder launch
    far = (s["pts"][:70] + F32(1000)).astype(F32)
    r = eng.query_map(s["t"], s["codes"], far)
    assert np.all(r["obj"] == -1) and np.all(np.isposinf(r["dist"])) and np.isfinite(r["bound"]).all()
    assert eng.query_stats() == {"rows": 0, "tiles": 0, "chunks": 0, "passes": 1}


def test_a_nan_point_disturbs_no_other_point(eng):
    s = scene3(eng)
    good = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    for bad in (np.nan, np.inf):
        q = s["pts"].copy()
        q[70, 1] = bad                                      # a point of the overlap
        r = eng.query_map(s["t"], s["codes"], q, normals=True)
        keep = np.arange(300) != 70
        for k in ("obj", "dist", "bound", "normal"):
            assert r[k][keep].tobytes() == good[k][keep].tobytes(), k
        assert r["obj"][70] == -1 and np.isposinf(r["dist"][70]) and np.all(r["normal"][70] == 0)
        assert np.isnan(r["bound"][70]) if np.isnan(bad) else not np.isfinite(r["bound"][70])


def test_an_object_with_a_nan_code_never_wins(eng):
    s = scene3(eng)
    bad_code = s["codes"][1].copy()
    bad_code[5] = np.nan
    t = np.concatenate([s["t"], s["t"][1:2]])               # the bad object shares sphere 1, which holds more than 150 of the points
    three = eng.query_map(s["t"], s["codes"], s["pts"], normals=True)
    four = eng.query_map(t, s["codes"] + [bad_code], s["pts"], normals=True)
    assert np.array_equal(four["obj"], three["obj"]) and _bits_equal(four["dist"], three["dist"]) and _bits_equal(four["normal"], three["normal"])
    rt, sc, _ = Q.invert(t)
    assert _bits_equal(four["bound"], Q.candidates(rt, sc, s["pts"])[2])
    # alone, it owns nothing
    alone = eng.query_map(t[3:], [bad_code], s["pts"], normals=True)
    assert np.all(alone["obj"] == -1) and np.all(np.isposinf(alone["dist"])) and np.all(alone["normal"] == 0)
    assert eng.query_stats()["rows"] == int(s["exp"]["inside"][1].sum()) > 150


def test_refused_arguments_leave_the_handle_usable(eng):
    s = scene3(eng)
    lib = L.load()
    t = L.f32(s["t"]).reshape(3, 16)
    c = np.stack([L.code64(x) for x in s["codes"]])
    p = L.f32(s["pts"])
    n = p.shape[0]
    o, d, b, nr = np.zeros(n, np.int32), np.zeros(n, F32), np.zeros(n, F32), np.zeros((n, 3), F32)

    def call(h=eng._h, t_=t, c_=c, n_obj=3, p_=p, n_pts=n, flags=0, o_=o, d_=d, b_=b, nr_=None):
        return lib.dsp_map_query(h, L.ptr(t_), L.ptr(c_), n_obj, L.ptr(p_), n_pts, flags, L.ptr(o_, L.c_i32p), L.ptr(d_), L.ptr(b_), L.ptr(nr_))

    assert call() == 0 and call(flags=1, nr_=nr) == 0
    for kw in (dict(flags=2), dict(flags=3, nr_=nr), dict(flags=1), dict(nr_=nr), dict(n_obj=-1), dict(n_pts=-1), dict(o_=None), dict(d_=None),
               dict(b_=None), dict(p_=None), dict(t_=None), dict(c_=None)):
        assert call(**kw) == -1, kw
    for what in ("sheared", "bottom", "nan", "zero"):
        bad = s["t"].copy()
        if what == "sheared":
            bad[1, :3, :3] = bad[1, :3, :3] @ np.array([[1, 0.01, 0], [0, 1, 0], [0, 0, 1]], F32)
        elif what == "bottom":
            bad[2, 3, 3] = 0.5
        elif what == "nan":
            bad[0, 0, 3] = np.nan
        else:
            bad[1, :3, :3] = 0
        assert call(t_=L.f32(bad).reshape(3, 16)) == -1, what
        with pytest.raises(L.DspError, match="pose"):
            eng.query_map(bad, s["codes"], s["pts"])
    with pytest.raises(ValueError):
        eng.query_map(s["t"], s["codes"][:2], s["pts"])
    _same(eng.query_map(s["t"], s["codes"], s["pts"], normals=True), s["exp"], keys=("obj", "dist", "bound", "normal"))


def test_a_32d_decoder(chairs32_decoder):
    e = _engine(chairs32_decoder)
    try:
        rng = np.random.default_rng(50)
        t = Q.sim3(Q.random_rotations(rng, 2), [1.2, 0.7], [[0.0, 0.0, 0.0], [1.0, 0.5, 0.0]])
        codes = _codes(51, 2, 32)
        pts = np.concatenate([_world(t[o], _in_ball(rng, 60, 1.3)) for o in range(2)])
        exp = Q.expected(e, t, codes, pts, with_normals=True)
        assert (exp["inside"][0] & exp["inside"][1]).sum() >= 5
        res = e.query_map(t, codes, pts, normals=True)
        _same(res, exp, keys=("obj", "dist", "bound", "normal"))
        # only the first 32 entries of a 64-wide code row are read
        wide = [np.concatenate([c, np.full(32, 7.5, F32)]) for c in codes]
        _same(e.query_map(t, wide, pts, normals=True), exp, keys=("obj", "dist", "bound", "normal"))
    finally:
        e.close()


# ---- 9. allocation failure ---------------------------------------------------------------------------------------------------------------
def test_allocation_failure_leaves_the_handle_usable(eng, oracle_decoder):
    s = scene3(eng)
    e = _engine(oracle_decoder)            # a handle of its own: what it already holds decides which allocations are fresh
    try:
        for normals in (False, True):
            for nth in (0, 2, 5):
                e.trim()                    # an empty cache: the call's own arrays have to be allocated afresh
                e.fail_alloc(nth)
                with pytest.raises(L.DspError, match="out of device memory"):
                    e.query_map(s["t"], s["codes"], s["pts"], normals=normals)
                e.fail_alloc(-1)
                e.trim()
                _same(e.query_map(s["t"], s["codes"], s["pts"], normals=normals), s["exp"],
                      keys=("obj", "dist", "bound") + (("normal",) if normals else ()))
    finally:
        e.fail_alloc(-1)
        e.close()


# ---- 10. the map file, end to end --------------------------------------------------------------------------------------------------------
def test_query_map_tool_end_to_end(tmp_path, eng):
    import test_gpu_map_tools as T
    s = scene3(eng)
    rng = np.random.default_rng(52)
    t = np.concatenate([s["t"], Q.sim3(Q.random_rotations(rng, 1), [1.0], [[1.0, -1.0, 0.5]])])
    codes = s["codes"] + _codes(53, 1)
    ids = [12, 3, 40, 7]
    map_dir = tmp_path / "map"
    map_dir.mkdir()
    M.write_map_objects(str(map_dir / "MapObjects.txt"), [dict(id=i, pose=p, code=c) for i, p, c in zip(ids, t, codes)])
    objs = M.read_map_objects(str(map_dir / "MapObjects.txt"))
    assert [o["id"] for o in objs] == sorted(ids)
    np.save(str(tmp_path / "pts.npy"), s["pts"])
    out = str(tmp_path / "query.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "tools", "query_map.py"), "--config", T._config(tmp_path), "--map_dir", str(map_dir), "--points", str(tmp_path / "pts.npy"),
        "--normals", "--max_dist", "0.02", "--out", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    got = dict(np.load(out))
    want = M.query_points(eng, objs, s["pts"], normals=True)
    for k in ("obj", "id", "dist", "bound", "normal"):
        assert got[k].tobytes() == want[k].tobytes() and got[k].dtype == want[k].dtype, k
    assert set(np.unique(want["id"])) <= set(ids) | {-1} and (want["id"] >= 0).sum() > 150
    a = M.associate(want, 0.02)
    assert len(a) >= 2 and got["assoc_ids"].tolist() == sorted(a)
    for k, i in enumerate(got["assoc_ids"]):
        assert np.array_equal(got["assoc_pts"][got["assoc_off"][k]:got["assoc_off"][k + 1]], a[int(i)])
    # and the file's answer is the expected one for the poses and codes as the map file carries them
    exp = Q.expected(eng, np.stack([o["pose"] for o in objs]).astype(F32), [o["code"] for o in objs], s["pts"], with_normals=True)
    _same(want, exp, keys=("obj", "dist", "bound", "normal"))


# ---- build invariant ---------------------------------------------------------------------------------------------------------------------
def test_query_kernels_use_no_scratch():
    """The new kernels keep everything in registers and LDS: no scratch memory, no spills (the library's kernel report, build.check_isa)."""
    from dsp_slam_amd import build as B
    L.load()
    if not os.path.exists(os.path.join(B.OBJ_DIR, "query_kernels.hip.o")):
        pytest.skip("object files not kept on this box")
    rep = B.check_isa()
    mine = {k: v for k, v in rep["kernels"].items() if "k_query_" in k}
    assert len(mine) == 6, sorted(mine)
    for k, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
