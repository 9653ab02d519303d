"""GPU: ray casting against the object map (include/dsp_gn.h dsp_map_raycast): the first surface hit per world ray.

The expected values come from tests/raycast_ref.py: the numpy restatement of csrc/raycast_math.h's opening comment (pinned on the CPU by
tests/test_raycast_host.py) marches the pairs round by round and decodes each object's live samples with Engine.decode_sdf -- the normals
with Engine.sdf_jacobian -- at its own object-frame points.  Comparisons are bit for bit (obj, status; t, dist, normal by bits) and the
stats are compared exactly: the decoder forms are bit-identical across tile lists by the suite's own assertions, so no tolerance is needed.
Seeds are recorded where they were chosen: every scene below marches to an end within its max_steps where the test says so (asserted on
the reference).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import query_ref as Q
import raycast_ref as R
from conftest import ROOT
from dsp_slam_amd import engine as E, _lib as L, fixtures
from dsp_slam_amd import map_objects as M

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("obj", "t", "dist", "status", "normal")
STEPS = 48


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _codes(seed, n, code_len=64):
    return list(np.random.default_rng(seed).uniform(-0.3, 0.3, (n, code_len)).astype(F32))


def _bytes_equal(a, b, keys=KEYS):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def _same(got, want, stats=None):
    """Outputs bit for bit against the reference (NaN payloads aside there is no NaN in any output), and the stats exactly."""
    for k in ("obj", "status"):
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:10])
    for k in ("t", "dist", "normal"):
        if want[k] is None:
            assert got[k] is None, k
            continue
        a, b = np.ascontiguousarray(got[k], F32).view(np.uint32), np.ascontiguousarray(want[k], F32).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (k, np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1))[:10])
    if stats is not None:
        assert stats == R.stats_of(want["stats"]), (stats, R.stats_of(want["stats"]))


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.sqrt((u * u).sum(1))[:, None]


def _aimed(rng, t, n, reach, dist=2.5):
    """n rays from `dist` object radii out toward points within `reach` radii of the object's centre; directions of arbitrary length."""
    a, c = t[:3, :3].astype(np.float64), t[:3, 3].astype(np.float64)
    s = np.cbrt(np.linalg.det(a))
    org = c + s * dist * _unit(rng, n)
    tgt = c + s * reach * rng.uniform(0, 1, (n, 1)) ** (1 / 3) * _unit(rng, n)
    return org.astype(F32), ((tgt - org) * rng.uniform(0.2, 3.0, (n, 1))).astype(F32)


# ---- the scene of tests 2 - 7: the three objects of the map-query tests, two of the spheres overlapping --------------------------------------
_SCENE = {}


def scene3(eng):
    """Poses, codes, 300 rays and the expected result with normals at max_steps 48; computed once, never modified.  Rays 0..99 come from
    beyond object 0 and look through it toward object 1, rays 100..199 the other way round, rays 200..299 look at object 2 or past it.
    Seed 71 (poses: 41 and codes: 42, as in the map-query tests)."""
    if not _SCENE:
        t = Q.sim3(Q.random_rotations(np.random.default_rng(41), 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [1.25, 0.3, -0.2], [4.0, -3.0, 1.0]])
        codes = _codes(42, 3)
        rng = np.random.default_rng(71)
        c = t[:, :3, 3].astype(np.float64)
        axis = (c[1] - c[0]) / np.linalg.norm(c[1] - c[0])
        m = 160                                                         # candidates per group; the first 100 that march to an end are kept
        o_a = c[0] - 2.5 * axis + 0.25 * rng.normal(size=(m, 3))
        d_a = (c[1] + 0.3 * rng.normal(size=(m, 3))) - o_a
        o_b = c[1] + 3.5 * axis + 0.25 * rng.normal(size=(m, 3))
        d_b = (c[0] + 0.2 * rng.normal(size=(m, 3))) - o_b
        o_c, d_c = _aimed(rng, t[2], m, 1.3)
        org = np.concatenate([o_a, o_b, o_c]).astype(F32)
        dirs = np.concatenate([d_a, d_b, d_c]).astype(F32)
        prm = dict(max_steps=STEPS)
        done = R.expected(eng, t, codes, org, dirs, prm)["exhausted_at"] == R.NONE32      # the reference marches every pair of the ray to an end
        keep = np.concatenate([k * m + np.flatnonzero(done[k * m:(k + 1) * m])[:100] for k in range(3)])
        assert keep.size == 300, [int(done[k * m:(k + 1) * m].sum()) for k in range(3)]
        org, dirs = org[keep], dirs[keep]
        _SCENE.update(t=t, codes=codes, org=org, dirs=dirs, prm=prm, exp=R.expected(eng, t, codes, org, dirs, prm, with_normals=True))
        assert _SCENE["exp"]["stats"]["exhausted"] == 0
    return _SCENE


# ---- 1. one object, identity pose --------------------------------------------------------------------------------------------------------
def test_one_object_identity_pose(eng):
    rng = np.random.default_rng(72)
    code = _codes(44, 1)[0]
    t = np.eye(4, dtype=F32)[None]
    org, dirs = _aimed(rng, t[0], 300, 0.95)
    exp = R.expected(eng, t, [code], org, dirs, dict(max_steps=STEPS))
    n_hit, n_miss = int((exp["status"] == R.HIT).sum()), int((exp["status"] == R.MISS).sum())
    print("hits %d, misses %d, undecided %d, rows per round %s" % (n_hit, n_miss, 300 - n_hit - n_miss, exp["stats"]["rows_per_round"]))
    assert n_hit >= 30 and n_miss >= 30 and exp["stats"]["pairs"] == 300
    res = eng.cast_rays(t, [code], org, dirs, max_steps=STEPS)
    _same(res, exp, eng.raycast_stats())
    assert (res["status"] == R.HIT).sum() == n_hit and (res["status"] == R.MISS).sum() == n_miss
    hit = np.flatnonzero(res["status"] == R.HIT)
    assert np.all(res["obj"][hit] == 0) and np.all(res["dist"][hit] <= F32(1e-3)) and np.all(np.isposinf(res["t"][res["obj"] < 0]))
    # with the identity pose the object-frame sample is fmaf(t, u, o): the map query at that point decodes the same row
    g = exp["geometry"]
    pw = R.sample(org[hit], g["u"][hit], res["t"][hit])
    q = eng.query_map(t, [code], pw)
    same_point = (pw.view(np.uint32) == R.sample(g["o_o"][0, hit], g["d_o"][0, hit], res["t"][hit]).view(np.uint32)).all(1)
    assert same_point.all()
    assert np.array_equal(q["dist"][same_point].view(np.uint32), res["dist"][hit][same_point].view(np.uint32))
    assert np.all(q["dist"][~same_point] <= F32(1e-3)) and np.all(q["obj"] == 0)


# ---- 2. three objects, occlusion ---------------------------------------------------------------------------------------------------------
def test_three_objects_the_nearer_surface_wins(eng):
    s = scene3(eng)
    exp = s["exp"]
    two = exp["stats"]["pairs_per_ray"] >= 2
    print("rays with two pairs %d, retired pairs %d, exhausted %d, rows per round %s" % (
        two.sum(), exp["stats"]["retired"], exp["stats"]["exhausted"], exp["stats"]["rows_per_round"]))
    assert two.sum() >= 20 and exp["stats"]["retired"] >= 1
    res = eng.cast_rays(s["t"], s["codes"], s["org"], s["dirs"], normals=True, **s["prm"])
    _same(res, exp, eng.raycast_stats())
    # rays through both spheres: object 0 is in front one way round, object 1 the other way
    a, b = np.arange(300) < 100, (np.arange(300) >= 100) & (np.arange(300) < 200)
    front_a, front_b = res["obj"][a & two & (res["obj"] >= 0)], res["obj"][b & two & (res["obj"] >= 0)]
    assert (front_a == 0).sum() >= 10 and (front_b == 1).sum() >= 10
    assert (res["obj"] == 2).sum() >= 10 and set(np.unique(res["obj"])) == {-1, 0, 1, 2}
    hit = res["obj"] >= 0
    length = np.sqrt((res["normal"][hit].astype(np.float64) ** 2).sum(1))
    assert np.abs(length - 1).max() <= 2 * 2.0 ** -23 and np.all(res["normal"][~hit] == 0)
    # a hit surface faces the ray
    u = exp["geometry"]["u"].astype(np.float64)
    assert ((res["normal"][hit] * u[hit]).sum(1) < 0).mean() > 0.75
    # the flag changes no other output
    _bytes_equal(eng.cast_rays(s["t"], s["codes"], s["org"], s["dirs"], **s["prm"]), res, keys=("obj", "t", "dist", "status"))


# ---- 3. the same object listed twice -----------------------------------------------------------------------------------------------------
def test_the_same_object_twice_reports_the_lower_index(eng):
    s = scene3(eng)
    t = np.stack([s["t"][2], s["t"][1], s["t"][1], s["t"][2]])
    codes = [s["codes"][2], s["codes"][1], s["codes"][1], s["codes"][2]]
    res = eng.cast_rays(t, codes, s["org"], s["dirs"], normals=True, **s["prm"])
    st = eng.raycast_stats()
    alone = eng.cast_rays(t[:2], codes[:2], s["org"], s["dirs"], normals=True, **s["prm"])
    _bytes_equal(res, alone)
    assert set(np.unique(res["obj"])) == {-1, 0, 1} and (res["obj"] >= 0).sum() > 50
    _same(res, R.expected(eng, t, codes, s["org"], s["dirs"], s["prm"], with_normals=True), st)


# ---- 4. raggedness, pass cuts, repetition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_counts_and_pass_cuts_return_identical_bytes(eng, n):
    s = scene3(eng)
    lib = L.load()
    pick = np.random.default_rng(73).permutation(300)[:n]          # seed 73: rays of all three groups in every count but 1
    org, dirs = s["org"][pick], s["dirs"][pick]
    whole = eng.cast_rays(s["t"], s["codes"], org, dirs, normals=True, **s["prm"])
    st = eng.raycast_stats()
    for k in ("obj", "t", "dist", "status", "normal"):                  # a subset of the rays returns the subset of the results
        assert whole[k].tobytes() == s["exp"][k][pick].tobytes(), k
    _bytes_equal(eng.cast_rays(s["t"], s["codes"], org, dirs, normals=True, **s["prm"]), whole)
    assert eng.raycast_stats() == st and st["passes"] == (1 if st["pairs"] else 0)
    for rows in (64, 100):
        assert lib.dsp_debug_query_chunk_rows(eng._h, rows) == 0
        try:
            cut = eng.cast_rays(s["t"], s["codes"], org, dirs, normals=True, **s["prm"])
            st_cut = eng.raycast_stats()
        finally:
            assert lib.dsp_debug_query_chunk_rows(eng._h, 0) == 0
        _bytes_equal(cut, whole)
        assert st_cut["pairs"] == st["pairs"] and st_cut["passes"] == -(-st["pairs"] // rows)
    if n == 257:
        assert st["pairs"] > 200                                        # several passes at either budget, cut inside objects
        exp = R.expected(eng, s["t"], s["codes"], org, dirs, s["prm"], with_normals=True, budget=100)
        assert lib.dsp_debug_query_chunk_rows(eng._h, 100) == 0
        try:
            _same(eng.cast_rays(s["t"], s["codes"], org, dirs, normals=True, **s["prm"]), exp, eng.raycast_stats())
        finally:
            assert lib.dsp_debug_query_chunk_rows(eng._h, 0) == 0


# ---- 5. rays that start inside a surface; t_min and t_max --------------------------------------------------------------------------------
def test_starts_inside_a_surface_and_parameter_clipping(eng):
    s = scene3(eng)
    rng = np.random.default_rng(74)
    t, codes = s["t"], s["codes"]
    c0 = t[0, :3, 3].astype(np.float64)
    # 60 rays from within 0.04 of object 0's centre, which lies inside its shape
    org = (c0 + 0.04 * _unit(rng, 60) * rng.uniform(0, 1, (60, 1))).astype(F32)
    dirs = _unit(rng, 60).astype(F32)
    exp = R.expected(eng, t, codes, org, dirs, s["prm"], with_normals=True)
    res = eng.cast_rays(t, codes, org, dirs, normals=True, **s["prm"])
    _same(res, exp, eng.raycast_stats())
    assert np.all(res["status"] == R.HIT) and np.all(res["obj"] == 0) and np.all(res["t"] == 0) and np.all(res["dist"] < 0)
    # object 0 alone (from some directions object 1 stands in front of it).  Rays from outside toward the centre: t_min at the centre's
    # distance starts the march beyond the first surface, inside the shape
    t, codes = t[:1], codes[:1]
    o2, d2 = _aimed(rng, t[0], 60, 0.02)
    far = np.sqrt(((c0 - o2.astype(np.float64)) ** 2).sum(1))
    t_min = float(F32(far.max()))
    plain = eng.cast_rays(t, codes, o2, d2, **s["prm"])
    exp = R.expected(eng, t, codes, o2, d2, s["prm"])
    _same(plain, exp, eng.raycast_stats())
    assert np.all(plain["status"] == R.HIT) and np.all(plain["obj"] == 0) and np.all(plain["t"] < F32(t_min))
    prm = dict(s["prm"], t_min=t_min)
    late = eng.cast_rays(t, codes, o2, d2, **prm)
    _same(late, R.expected(eng, t, codes, o2, d2, prm), eng.raycast_stats())
    assert np.all(late["obj"] == 0) and np.all(late["t"] == F32(t_min)) and np.all(late["dist"] < 0)
    # t_max short of the first surface, for the rays that hit well behind the last sphere entry (the shape reaches the sphere along its long
    # axis, where a ray hits as it enters): the pairs exist (every sphere is entered) and every ray misses
    entry = exp["geometry"]["t0"][0].max()
    sel = plain["t"] > entry + F32(0.05)
    assert sel.sum() >= 20
    prm = dict(s["prm"], t_max=float(entry + F32(0.025)))
    short = eng.cast_rays(t, codes, o2[sel], d2[sel], **prm)
    _same(short, R.expected(eng, t, codes, o2[sel], d2[sel], prm), eng.raycast_stats())
    assert eng.raycast_stats()["pairs"] == sel.sum() and eng.raycast_stats()["rows"] >= sel.sum()
    assert np.all(short["status"] == R.MISS) and np.all(short["obj"] == -1) and np.all(np.isposinf(short["dist"]))


# ---- 6. exhaustion -----------------------------------------------------------------------------------------------------------------------
def test_exhausted_pairs_make_rays_undecided(eng):
    s = scene3(eng)
    prm = dict(max_steps=2)
    exp = R.expected(eng, s["t"], s["codes"], s["org"], s["dirs"], prm, with_normals=True)
    und = exp["status"] == R.UNDECIDED
    print("max_steps 2: exhausted pairs %d, undecided rays %d (with a winner: %d)" % (exp["stats"]["exhausted"], und.sum(), (und & (exp["obj"] >= 0)).sum()))
    assert exp["stats"]["exhausted"] >= 50 and und.sum() >= 50 and exp["stats"]["rounds"] == 2
    res = eng.cast_rays(s["t"], s["codes"], s["org"], s["dirs"], normals=True, **prm)
    _same(res, exp, eng.raycast_stats())
    assert np.array_equal(res["status"] == R.UNDECIDED, und) and eng.raycast_stats()["exhausted"] == exp["stats"]["exhausted"]
    # with the larger cap the same rays resolve
    full = s["exp"]
    assert np.all(full["status"][und] != R.UNDECIDED) and full["stats"]["exhausted"] == 0
    res = eng.cast_rays(s["t"], s["codes"], s["org"], s["dirs"], normals=True, **s["prm"])
    assert np.array_equal(res["status"], full["status"]) and eng.raycast_stats()["exhausted"] == 0


# ---- 7. void rays, an object with a NaN code; the handle stays usable ---------------------------------------------------------------------
def test_void_rays_and_a_nan_code_disturb_nothing(eng):
    s = scene3(eng)
    good = s["exp"]
    org, dirs = s["org"].copy(), s["dirs"].copy()
    bad = [5, 64, 150, 151, 299]
    org[5, 1] = np.nan
    dirs[64] = 0
    dirs[150, 2] = np.inf
    org[151, 0] = -np.inf
    dirs[299] = np.nan
    bad_code = s["codes"][1].copy()
    bad_code[5] = np.nan
    t = np.concatenate([s["t"], s["t"][1:2]])                          # the bad object shares sphere 1
    codes = s["codes"] + [bad_code]
    res = eng.cast_rays(t, codes, org, dirs, normals=True, **s["prm"])
    st = eng.raycast_stats()
    keep = np.ones(300, bool)
    keep[bad] = False
    for k in KEYS:
        assert res[k][keep].tobytes() == good[k][keep].tobytes(), k
    assert np.all(res["obj"][bad] == -1) and np.all(np.isposinf(res["t"][bad])) and np.all(np.isposinf(res["dist"][bad]))
    assert np.all(res["status"][bad] == R.MISS) and np.all(res["normal"][bad] == 0)
    _same(res, R.expected(eng, t, codes, org, dirs, s["prm"], with_normals=True), st)
    # the very next call on the handle is a plain map query, checked against its own expectation
    pts = (s["t"][0, :3, 3] + 0.3 * _unit(np.random.default_rng(75), 50)).astype(F32)
    q = eng.query_map(s["t"], s["codes"], pts)
    want = Q.expected(eng, s["t"], s["codes"], pts)
    assert np.array_equal(q["obj"], want["obj"]) and np.array_equal(q["dist"].view(np.uint32), want["dist"].view(np.uint32)) and (q["obj"] >= 0).all()


# ---- 8. edges ----------------------------------------------------------------------------------------------------------------------------
def test_no_rays_no_objects_and_refusals(eng):
    s = scene3(eng)
    r = eng.cast_rays(np.zeros((0, 4, 4), F32), [], s["org"][:7], s["dirs"][:7], normals=True)
    assert np.all(r["obj"] == -1) and np.all(np.isposinf(r["t"])) and np.all(np.isposinf(r["dist"])) and np.all(r["status"] == R.MISS)
    assert np.all(r["normal"] == 0) and eng.raycast_stats() == dict(pairs=0, rows=0, tiles=0, rounds=0, passes=0, exhausted=0)
    r = eng.cast_rays(s["t"], s["codes"], np.zeros((0, 3), F32), np.zeros((0, 3), F32), normals=True)
    assert r["obj"].shape == (0,) and r["normal"].shape == (0, 3) and r["status"].dtype == np.int32
    lib = L.load()
    prm = E.Engine.raycast_params()
    assert lib.dsp_map_raycast(eng._h, None, None, 0, None, None, 0, L.C.byref(prm), 0, None, None, None, None, None) == 0
    # rays that look away from everything: no pair, no decoder launch
    far = eng.cast_rays(s["t"], s["codes"], s["org"][:70] + F32(1000), np.tile(np.array([1, 0, 0], F32), (70, 1)))
    assert np.all(far["obj"] == -1) and np.all(far["status"] == R.MISS)
    assert eng.raycast_stats() == dict(pairs=0, rows=0, tiles=0, rounds=0, passes=0, exhausted=0)
    # refusals
    t = L.f32(s["t"]).reshape(3, 16)
    c = np.stack([L.code64(x) for x in s["codes"]])
    o, d = L.f32(s["org"]), L.f32(s["dirs"])
    n = o.shape[0]
    ob, st, tt, dd, nr = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, F32), np.zeros(n, F32), np.zeros((n, 3), F32)

    def call(t_=t, c_=c, n_obj=3, o_=o, d_=d, n_=n, p_=prm, flags=0, ob_=ob, tt_=tt, dd_=dd, st_=st, nr_=None):
        return lib.dsp_map_raycast(eng._h, L.ptr(t_), L.ptr(c_), n_obj, L.ptr(o_), L.ptr(d_), n_, None if p_ is None else L.C.byref(p_), flags,
                                   L.ptr(ob_, L.c_i32p), L.ptr(tt_), L.ptr(dd_), L.ptr(st_, L.c_i32p), L.ptr(nr_))

    for kw in (dict(flags=2), dict(flags=3, nr_=nr), dict(flags=1), dict(nr_=nr), dict(n_obj=-1), dict(n_=-1), dict(ob_=None), dict(tt_=None),
               dict(dd_=None), dict(st_=None), dict(o_=None), dict(d_=None), dict(t_=None), dict(c_=None), dict(p_=None),
               dict(p_=E.Engine.raycast_params(eps=0.0)), dict(p_=E.Engine.raycast_params(max_steps=5000))):
        assert call(**kw) == -1, kw
    with pytest.raises(L.DspError, match="eps"):
        eng.cast_rays(s["t"], s["codes"], s["org"], s["dirs"], eps=-1.0)
    with pytest.raises(TypeError):
        eng.cast_rays(s["t"], s["codes"], s["org"], s["dirs"], epsilon=1.0)
    bad = s["t"].copy()
    bad[1, :3, :3] = 0
    with pytest.raises(L.DspError, match="pose"):
        eng.cast_rays(bad, s["codes"], s["org"], s["dirs"])
    assert call(flags=1, nr_=nr) == 0
    _bytes_equal(eng.cast_rays(s["t"], s["codes"], s["org"], s["dirs"], normals=True, **s["prm"]), s["exp"])


# ---- 9. the image, and the tool ----------------------------------------------------------------------------------------------------------
def test_render_and_the_tool(tmp_path, eng):
    s = scene3(eng)
    ids = [12, 3, 40]
    path = str(tmp_path / "MapObjects.txt")
    M.write_map_objects(path, [dict(id=i, pose=p, code=c) for i, p, c in zip(ids, s["t"], s["codes"])])
    objs = M.read_map_objects(path)
    assert [o["id"] for o in objs] == sorted(ids)
    # a camera 4 units from the overlapping pair, looking at it (x right, y down, z forward)
    z = np.array([0.6, 0.15, -0.1]) - np.array([-1.5, -3.0, 2.0])
    z /= np.linalg.norm(z)
    x = np.cross([0, 0, 1.0], z)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, [-1.5, -3.0, 2.0]
    W, H, K = 24, 16, (20.0, 20.0, 11.5, 7.5)
    img = M.render(eng, objs, K, T, W, H, normals=True, max_steps=STEPS)
    org, dirs, cos = M.pixel_rays(K, T, W, H)
    flat = M.cast_rays(eng, objs, org, dirs, normals=True, max_steps=STEPS)
    for k in ("obj", "id", "status", "t", "dist"):
        assert img[k].shape == (H, W) and img[k].tobytes() == flat[k].tobytes(), k
    assert img["normal"].shape == (H, W, 3) and img["normal"].tobytes() == flat["normal"].tobytes()
    hit = flat["obj"] >= 0
    assert 40 <= hit.sum() < W * H and set(np.unique(flat["id"])) <= set(ids) | {-1}
    want = np.where(hit, flat["t"].astype(np.float64) * cos, np.inf).astype(F32)
    assert img["depth"].dtype == F32 and img["depth"].tobytes() == want.tobytes() and np.all(img["depth"].reshape(-1)[hit] <= flat["t"][hit])
    # the tool, once, in a child process
    cars = fixtures.materialize_decoder_dir("cars", str(tmp_path / "cars_64"))
    np.save(str(tmp_path / "pose.npy"), T)
    out = str(tmp_path / "render.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "tools", "render_map.py"), "--map", path, "--decoder", cars, "--intrinsics"] + [repr(v) for v in K] + [
        "--size", str(W), str(H), "--pose", str(tmp_path / "pose.npy"), "--normals", "--max-steps", str(STEPS), "--out", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    got = dict(np.load(out))
    for k in ("depth", "id", "obj", "status", "t", "dist", "normal"):
        assert got[k].dtype == img[k].dtype and got[k].tobytes() == img[k].tobytes(), k


# ---- 10. rays at surface points ----------------------------------------------------------------------------------------------------------
def test_rays_toward_projected_surface_points_hit_object_0(eng):
    s = scene3(eng)
    rng = np.random.default_rng(76)
    t0 = s["t"][0].astype(np.float64)
    scale = np.cbrt(np.linalg.det(t0[:3, :3]))
    start = 0.35 * _unit(rng, 100)
    sp = eng.surface_points([s["codes"][0]], [start.astype(F32)], steps=8)[0]
    assert np.abs(sp["sdf"]).max() < 1e-4
    p_w = sp["vertices"].astype(np.float64) @ t0[:3, :3].T + t0[:3, 3]
    n_w = sp["normals"].astype(np.float64) @ (t0[:3, :3] / scale).T
    org = (p_w + 1.5 * scale * n_w).astype(F32)
    dirs = (p_w - org.astype(np.float64)).astype(F32)
    # only object 0: the other spheres must not occlude a ray that starts 1.5 s out
    exp = R.expected(eng, s["t"][:1], s["codes"][:1], org, dirs, s["prm"], with_normals=True)
    res = eng.cast_rays(s["t"][:1], s["codes"][:1], org, dirs, normals=True, **s["prm"])
    _same(res, exp, eng.raycast_stats())
    assert np.all(res["status"] == R.HIT) and np.all(res["obj"] == 0)
    over = res["t"].astype(np.float64) - 1.5 * scale
    print("t_hit - t_true over 100 surface rays: min %.2e, median %.2e, max %.2e" % (over.min(), np.median(over), over.max()))
