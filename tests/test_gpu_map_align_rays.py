"""GPU: ray alignment (include/dsp_gn.h dsp_map_align_rays): projective SE(3) Gauss-Newton of measured depth rays against the ray-cast map.

The expected values come from tests/align_rays_ref.py (pinned on the CPU by tests/test_align_rays_host.py) composed with what existed
before: tests/raycast_ref.py marches every hypothesis' rays through Engine.decode_sdf, Engine.sdf_jacobian gives the winners' rows at the
restatement's own hit samples, tests/align_ref.py the rows, the tree and the loop.  Evaluations are compared bit for bit; a pose reached by
a step to 1e-14 (exp_se3's sin / cos).

Observations are made by Engine.cast_rays at T_TRUE with eps 1e-5 and 256 steps and moved to the sensor frame; the alignment casts with
64 steps and the default eps 1e-3.
"""
import numpy as np
import pytest

import align_rays_ref as AR
import align_ref as A
import query_ref as Q
import raycast_ref as R
from conftest import parity_log
from dsp_slam_amd import engine as E, _lib as L
from test_align_rays_host import aimed_rays

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MAX_DIST, HUBER, MAX_GAP = 0.3, 0.05, 0.6
RC = dict(max_steps=64)
STEP = (1e-3, 4.0, 0.5, 1e-9, 1e6)
T_TRUE = A.rigid(A.axis_angle([0.3, -1.0, 0.5], 0.7), [0.5, -1.5, 2.0])


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _u64(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def _same64(a, b):
    return a.shape == b.shape and bool(np.array_equal(_u64(a), _u64(b)))


def _same32(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def observe(eng, t, codes, T_true, dirs_s, per_obj):
    """The cast of sensor-frame directions from the sensor origin at T_true (eps 1e-5, 256 steps): the first per_obj hits of every object
    -> pts_s (float32, sensor frame), the object seen, the directions kept."""
    dirs_w = (dirs_s @ T_true[:3, :3].T).astype(F32)
    org_w = np.broadcast_to(T_true[:3, 3].astype(F32), dirs_w.shape).copy()
    c = eng.cast_rays(t, codes, org_w, dirs_w, eps=1e-5, max_steps=256)
    keep = np.concatenate([np.flatnonzero((c["obj"] == o) & (c["status"] == L.RAYCAST_HIT))[:per_obj] for o in range(len(codes))])
    u = dirs_w[keep].astype(F64)
    u /= np.sqrt((u * u).sum(1))[:, None]
    world = org_w[keep].astype(F64) + u * c["t"][keep].astype(F64)[:, None]
    inv = np.linalg.inv(T_true)
    return (world @ inv[:3, :3].T + inv[:3, 3]).astype(F32), c["obj"][keep], dirs_s[keep], world


_SCENE, _SCENE2 = {}, {}


def scene(eng):
    """The segmented scene: the three objects of tests/test_gpu_map_align.py (their spheres do not overlap) seen from T_TRUE by rays aimed
    at them, 100 hits per object; the start poses; computed once, never modified."""
    if not _SCENE:
        rng = np.random.default_rng(7)
        t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [2.6, 0.3, -0.2], [4.0, -3.0, 1.0]])
        codes = list(rng.uniform(-0.3, 0.3, (3, 64)).astype(F32))
        pts, seen, dirs, world = observe(eng, t, codes, T_TRUE, aimed_rays(rng, t, T_TRUE, 250), 100)
        assert pts.shape == (300, 3), pts.shape
        centre = world.mean(0)
        near, far = A.offset_pose(rng, T_TRUE, 5.0, 0.05, centre), A.offset_pose(rng, T_TRUE, 30.0, 0.3, centre)
        mid = A.offset_pose(rng, T_TRUE, 20.0, 0.2, centre)
        w = rng.uniform(0.0, 2.0, 300).astype(F32)
        w[rng.permutation(300)[:20]] = 0.0
        _SCENE.update(t=t, codes=codes, map=A.Map(t, codes), pts=pts, seen=seen, dirs=dirs, centre=centre, near=near, far=far, mid=mid, w=w)
    return _SCENE


def scene2(eng):
    """The overlapping layout of tests/test_gpu_map_query.py (spheres 0 and 1 overlap), seen along the line through the two centres from
    the side of object 0: object 0 stands in front of object 1, whose rim shows around it.  290 rays that see what they measured, and up
    to 10 GRAZING rays: rays that measured object 1 (the eps 1e-5 cast) after passing object 0 within the alignment's eps of 1e-3, so that
    the map cast as the alignment casts it shows object 0 in front of what they measured.  They are searched among 60 000 candidates."""
    if not _SCENE2:
        rng = np.random.default_rng(41)
        t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [1.25, 0.3, -0.2], [4.0, -3.0, 1.0]])[:2]
        codes = list(np.random.default_rng(42).uniform(-0.3, 0.3, (3, 64)).astype(F32))[:2]
        c0, c1 = t[0, :3, 3].astype(F64), t[1, :3, 3].astype(F64)
        view = (c1 - c0) / np.sqrt(((c1 - c0) ** 2).sum())
        x = np.cross([0.0, 0.0, 1.0], view)
        x /= np.sqrt((x * x).sum())
        T_true = A.rigid(np.stack([x, np.cross(view, x), view], 1), c0 - 4.0 * view)     # the camera looks along +z = view, object 0 first
        dirs = np.concatenate([aimed_rays(rng, t, T_true, 400), aimed_rays(rng, t[:1], T_true, 60000, spread=1.0)])
        dirs_w = (dirs @ T_true[:3, :3].T).astype(F32)
        org_w = np.broadcast_to(T_true[:3, 3].astype(F32), dirs_w.shape).copy()
        fine = eng.cast_rays(t, codes, org_w, dirs_w, eps=1e-5, max_steps=256)
        coarse = eng.cast_rays(t, codes, org_w, dirs_w, **RC)
        hit = (fine["status"] == L.RAYCAST_HIT) & (coarse["status"] == L.RAYCAST_HIT)
        with np.errstate(invalid="ignore"):             # inf - inf where neither cast hits
            graze = np.flatnonzero(hit & (fine["obj"] == 1) & (coarse["obj"] == 0) & (fine["t"] - coarse["t"] < 0.9 * MAX_GAP))[:10]
        plain = hit & (fine["obj"] == coarse["obj"]) & (np.arange(dirs.shape[0]) < 800)
        keep = np.concatenate([np.flatnonzero(plain & (fine["obj"] == 0))[:150], np.flatnonzero(plain & (fine["obj"] == 1))[:140 + 10 - graze.size], graze])
        assert keep.size == 300, (keep.size, graze.size)
        u = dirs_w[keep].astype(F64)
        u /= np.sqrt((u * u).sum(1))[:, None]
        world = org_w[keep].astype(F64) + u * fine["t"][keep].astype(F64)[:, None]
        inv = np.linalg.inv(T_true)
        pts = (world @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
        _SCENE2.update(t=t, codes=codes, map=A.Map(t, codes), pts=pts, seen=fine["obj"][keep], n_graze=int(graze.size), T_true=T_true, view=view,
                       centre=world.mean(0))
    return _SCENE2


def _ref_eval(eng, s, T, pts=None, w=None, org=None, max_gap=MAX_GAP, budget=None):
    return AR.evaluate(T, s["pts"] if pts is None else pts, org, w, eng, s["map"], s["codes"], HUBER, MAX_DIST, max_gap, RC, budget)


def _align(eng, s, hyp, pts=None, weights=None, origins=None, max_gap=MAX_GAP, **kw):
    kw.setdefault("max_dist", MAX_DIST)
    kw.setdefault("huber", HUBER)
    return eng.align_rays_to_map(s["t"], s["codes"], s["pts"] if pts is None else pts, hyp, origins=origins, weights=weights, per_ray=True, max_gap=max_gap,
                                 raycast=RC, **kw)


def _record_is(res, k, ev):
    """hypothesis k's returned record is the reference evaluation ev, bit for bit"""
    assert _same64(res["information"][k], A.full_h(ev["sums"])), k
    assert _same64(res["b"][k], ev["sums"][A.IDX_B:A.IDX_B + 6]), k
    assert _same64(res["cost"][k:k + 1], np.array([ev["cost"]])), (k, res["cost"][k], ev["cost"])
    assert res["n_used"][k] == ev["n_used"] and _same64(res["sum_w"][k:k + 1], ev["sums"][A.IDX_W:A.IDX_W + 1]), k


def _rays_are(res, k, ev):
    assert np.array_equal(res["obj"][k], ev["obj"]) and _same32(res["dist"][k], ev["dist"]), k
    assert _same32(res["t"][k], ev["t"]) and np.array_equal(res["status_ray"][k], ev["status"]), k


RESULT_KEYS = ("pose", "status", "evaluations", "steps", "cost0", "cost", "n_used", "sum_w", "lambda", "information", "b", "obj", "dist", "t", "status_ray")


def _bytes(res, k=None, trace=False):
    sl = slice(None) if k is None else slice(k, k + 1)
    out = [np.ascontiguousarray(res[key][sl]).tobytes() for key in RESULT_KEYS]
    if trace:
        out += [np.ascontiguousarray(res["trace"][key][sl]).tobytes() for key in sorted(res["trace"])]
    return out


# ---- 4. one evaluation, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_one_evaluation_is_the_reference_bit_for_bit(eng, n, weighted):
    s = scene(eng)
    idx = np.arange(300) if n == 300 else np.sort(np.random.default_rng(n).permutation(300)[:n])
    pts = s["pts"][idx]
    w = s["w"][idx].copy() if weighted else None
    if weighted and n == 1:
        w[0] = 1.5
    hyp = np.stack([T_TRUE, s["near"], s["far"]])
    res = _align(eng, s, hyp, pts=pts, weights=w, iterations=1, trans_tol=0.0, rot_tol=0.0)
    assert res["evaluations"].tolist() == [1, 1, 1] and res["steps"].tolist() == [0, 0, 0] and eng.align_rays_stats()["evaluations"] == 1
    used = []
    for k in range(3):
        pw, ow, dirv = AR.build(hyp[k], pts)
        ex = R.expected(eng, s["t"], s["codes"], ow, dirv, RC)
        assert np.array_equal(res["t"][k].view(np.uint32), ex["t"].view(np.uint32)) and np.array_equal(res["status_ray"][k], ex["status"]), k
        ev = _ref_eval(eng, s, hyp[k], pts, w)
        assert np.array_equal(ev["cast_obj"], ex["obj"])
        assert np.array_equal(res["obj"][k], np.where(ev["obj"] >= 0, ex["obj"], -1)), k
        _record_is(res, k, ev)
        _rays_are(res, k, ev)
        assert _same64(res["pose"][k], hyp[k]) and _same64(res["cost0"][k:k + 1], res["cost"][k:k + 1])
        assert res["status"][k] == (L.ALIGN_NO_SUPPORT if ev["n_used"] < 6 else L.ALIGN_OK)
        used.append(ev["n_used"])
    if n == 300:
        assert used[0] == (280 if weighted else 300) and used[2] < used[0], used        # at the true pose every ray sees what it measured
        assert res["best"] == 0


# ---- 5. every evaluation of a run --------------------------------------------------------------------------------------------------------
def _step_rule(costs):
    costs = np.ascontiguousarray(costs, F64)
    dec, lam = np.zeros(costs.shape[0], np.int32), np.zeros(costs.shape[0], F64)
    assert L.load().dsp_debug_step_rule(costs.shape[0], L.ptr(costs, L.c_f64p), *STEP, L.ptr(dec, L.c_i32p), L.ptr(lam, L.c_f64p)) == 0
    return dec, lam


@pytest.mark.parametrize("step_control", [True, False])
def test_every_evaluation_of_a_run_is_the_reference(eng, step_control):
    s = scene(eng)
    hyp = np.stack([s["near"], s["mid"]])
    kw = dict(step_control=STEP) if step_control else {}
    res = _align(eng, s, hyp, iterations=8, trans_tol=0.0, rot_tol=0.0, trace=True, **kw)
    tr = res["trace"]
    for k in range(2):
        n_ev = int(res["evaluations"][k])
        assert n_ev == 8 and np.all(tr["decision"][k] != 0) and _same64(tr["pose"][k, 0], hyp[k])
        acc = None
        for e in range(n_ev):
            ev = _ref_eval(eng, s, tr["pose"][k, e])
            assert ev["n_used"] >= 6                                           # the replay of the rule below assumes support throughout
            assert _same64(tr["H"][k, e], A.full_h(ev["sums"])) and _same64(tr["b"][k, e], ev["sums"][A.IDX_B:A.IDX_B + 6]), (k, e)
            assert _same64(tr["cost"][k, e:e + 1], np.array([ev["cost"]])) and tr["n_used"][k, e] == ev["n_used"], (k, e)
            if tr["decision"][k, e] == A.ACCEPTED:
                acc = dict(ev, pose=tr["pose"][k, e])
            xi = A.solve(A.full_h(acc["sums"]), acc["sums"][A.IDX_B:A.IDX_B + 6], 0.0, tr["lambda"][k, e])
            assert xi is not None and _same64(tr["xi"][k, e], xi), (k, e)
            if e + 1 < n_ev:
                nxt = A.apply_step(xi, acc["pose"])
                assert np.all(np.abs(tr["pose"][k, e + 1] - nxt) <= 1e-14 * np.maximum(1.0, np.abs(nxt))), (k, e)
        if step_control:
            dec, lam = _step_rule(tr["cost"][k])
            assert np.array_equal(tr["decision"][k], dec) and _same64(tr["lambda"][k], lam), k
        else:
            assert np.all(tr["decision"][k] == A.ACCEPTED) and not tr["lambda"][k].any()
        _record_is(res, k, acc)                                                # the returned state is the last accepted one
        _rays_are(res, k, acc)
        assert _same64(res["pose"][k], acc["pose"]) and res["steps"][k] == (tr["decision"][k, 1:] == A.ACCEPTED).sum()


# ---- 6. occlusion and free space ---------------------------------------------------------------------------------------------------------
def test_occlusion_and_free_space(eng):
    s = scene2(eng)
    T = s["T_true"]
    res = _align(eng, s, T[None], iterations=1)
    ev = _ref_eval(eng, s, T)
    _record_is(res, 0, ev)
    _rays_are(res, 0, ev)
    # every matched ray pairs with the FRONT surface: the first one along it in the map as the alignment casts it
    pw, ow, dirv = AR.build(T, s["pts"])
    front = eng.cast_rays(s["t"], s["codes"], ow, dirv, **RC)
    m = res["obj"][0] >= 0
    assert m.sum() >= 290 and np.array_equal(res["obj"][0][m], front["obj"][m]) and set(np.unique(res["obj"][0][m])) == {0, 1}
    plain = np.arange(300) < 300 - s["n_graze"]
    assert np.array_equal(res["obj"][0][m & plain], s["seen"][m & plain])               # ... which is the one they measured, the grazing rays aside
    # the point aligner at the same pose pairs a point with the smallest sdf s among the spheres that contain it, whatever stands in front of
    # it along the ray.  The count is the restatements' alone.
    pt = eng.align_to_map(s["t"], s["codes"], s["pts"], T[None], per_point=True, iterations=1, max_dist=MAX_DIST, huber=HUBER)
    decode = lambda o, p: (lambda v, g: (v, g[:, -3:]))(*eng.sdf_jacobian(s["codes"][o], p))
    pe = A.evaluate(T, s["pts"], None, s["map"], decode, HUBER, MAX_DIST)
    differ = int(((pe["obj"] >= 0) & (ev["obj"] >= 0) & (pe["obj"] != ev["obj"])).sum())
    got = int(((pt["obj"][0] >= 0) & m & (pt["obj"][0] != res["obj"][0])).sum())
    print("grazing rays found %d; rays whose front surface is not the point aligner's object: %d (restatement %d)" % (s["n_graze"], got, differ))
    assert differ >= 1 and got == differ
    # free space: the sensor moved 1.0 forward along its view.  The measured points now lie 1.0 further into the scene: object 0 and object 1
    # stand in front of them
    shifted = A.rigid(np.eye(3), 1.0 * s["view"]) @ T
    both = _align(eng, s, np.stack([T, shifted]), iterations=1)
    valid = np.isfinite(A.transform(shifted, s["pts"])).all(1)
    unmatched = [int((valid & (both["obj"][k] < 0)).sum()) for k in range(2)]
    print("unmatched valid rays / cost: true pose %d / %.3e, an object in front of the measured points %d / %.3e" % (
        unmatched[0], both["cost"][0], unmatched[1], both["cost"][1]))
    assert unmatched[1] > unmatched[0] and both["cost"][1] > both["cost"][0]
    _record_is(both, 1, _ref_eval(eng, s, shifted))


# ---- 7. the gap gate ---------------------------------------------------------------------------------------------------------------------
def test_the_gap_gate_ignores_the_background(eng):
    s = scene(eng)
    rng = np.random.default_rng(11)
    # background: more rays towards the objects whose measured depth is a constant 9, far behind every object
    u = aimed_rays(rng, s["t"], T_TRUE, 20)
    back = (u * 9.0).astype(F32)
    pts = np.concatenate([s["pts"], back])
    hyp = np.stack([T_TRUE, s["near"], s["far"]])
    kw = dict(iterations=1)
    plain = _align(eng, s, hyp, **kw)
    gated = _align(eng, s, hyp, pts=pts, **kw)
    assert _same64(gated["information"], plain["information"]) and _same64(gated["b"], plain["b"]) and np.array_equal(gated["n_used"], plain["n_used"])
    assert np.all(gated["obj"][:, 300:] == -1) and (gated["status_ray"][:, 300:] == L.RAYCAST_HIT).sum() >= 40      # they hit, far from depth 9
    assert np.all(gated["sum_w"] == plain["sum_w"] + 60.0) and np.all(gated["cost"] > plain["cost"])
    # weights of 0 on the background rows: sum_w and the cost are the plain call's too
    w = np.concatenate([np.ones(300, F32), np.zeros(60, F32)])
    ctl = _align(eng, s, hyp, pts=pts, weights=w, **kw)
    for key in ("information", "b", "cost", "sum_w"):
        assert _same64(ctl[key], plain[key]), key
    # without the gate the background reaches the system through grazing hits
    free = _align(eng, s, hyp, pts=pts, max_gap=np.inf, **kw)
    assert (free["obj"][:, 300:] >= 0).any() and not _same64(free["information"], plain["information"])
    _record_is(free, 1, _ref_eval(eng, s, hyp[1], pts, max_gap=np.inf))


# ---- 8. ended hypotheses cost nothing ----------------------------------------------------------------------------------------------------
def test_an_ended_hypothesis_costs_no_rows(eng):
    """With tolerances of 1e-2 the hypothesis at T_TRUE converges at its first evaluation (its first step is the eps remainder, below 1e-3);
    the 20-degree one runs on.  From the second evaluation on the cast's counts are those of the surviving hypothesis run alone."""
    s = scene(eng)
    hyp = np.stack([T_TRUE, s["mid"]])
    kw = dict(trans_tol=1e-2, rot_tol=1e-2, trace=True)
    res = _align(eng, s, hyp, iterations=6, **kw)
    st = eng.align_rays_stats()
    assert res["evaluations"][0] == 1 and res["status"][0] == L.ALIGN_CONVERGED and res["evaluations"][1] > 2
    assert st["evaluations"] == int(res["evaluations"][1])
    _align(eng, s, hyp, iterations=1, **kw)
    st1 = eng.align_rays_stats()
    alone = _align(eng, s, hyp[1:], iterations=6, **kw)
    sa = eng.align_rays_stats()
    _align(eng, s, hyp[1:], iterations=1, **kw)
    sa1 = eng.align_rays_stats()
    assert _bytes(res, 1, trace=True) == _bytes(alone, trace=True)
    for key in ("pairs", "rows", "tiles", "rounds", "exhausted"):
        assert st[key] - st1[key] == sa[key] - sa1[key] and (key == "exhausted" or sa[key] > sa1[key]), key
    assert st1["pairs"] > sa1["pairs"] and st1["rows"] > sa1["rows"]                  # the first evaluation did march both
    assert not res["trace"]["decision"][0, 1:].any() and not res["trace"]["pose"][0, 1:].any()
    assert _bytes(res, 0) == _bytes(_align(eng, s, hyp[:1], iterations=1, **kw))


# ---- 9. same bytes, whatever the cut -----------------------------------------------------------------------------------------------------
def test_the_cut_the_repeat_and_the_batch_return_the_same_bytes(eng):
    s = scene2(eng)
    lib = L.load()
    hyp = np.stack([s["T_true"], A.offset_pose(np.random.default_rng(3), s["T_true"], 2.0, 0.02, s["centre"])])
    kw = dict(iterations=3, trace=True, weights=np.random.default_rng(4).uniform(0.0, 2.0, 300).astype(F32), step_control=STEP)
    whole = _align(eng, s, hyp, **kw)
    st = eng.align_rays_stats()
    assert _bytes(whole, trace=True) == _bytes(_align(eng, s, hyp, **kw), trace=True)                      # repeated
    for k in range(2):
        assert _bytes(whole, k, trace=True) == _bytes(_align(eng, s, hyp[k:k + 1], **kw), trace=True), k   # alone against inside the batch
    assert st["passes"] == st["evaluations"] == 3
    for budget in (70, 257):           # pairs per pass: several passes, and the winners' rows (300 per hypothesis) across chunk borders
        assert lib.dsp_debug_query_chunk_rows(eng._h, budget) == 0
        try:
            cut = _align(eng, s, hyp, **kw)
            st2 = eng.align_rays_stats()
        finally:
            assert lib.dsp_debug_query_chunk_rows(eng._h, 0) == 0
        assert _bytes(cut, trace=True) == _bytes(whole, trace=True), budget
        assert st2["pairs"] == st["pairs"] and st2["passes"] > 2 * st["passes"], budget
    ev = _ref_eval(eng, s, hyp[1], w=kw["weights"], budget=70)
    assert _same64(whole["trace"]["H"][1, 0], A.full_h(ev["sums"])) and _same64(whole["trace"]["b"][1, 0], ev["sums"][A.IDX_B:A.IDX_B + 6])


# ---- 10. neighbours untouched ------------------------------------------------------------------------------------------------------------
def test_the_neighbours_are_unchanged_around_a_call(eng):
    s = scene(eng)
    pw, ow, dirv = AR.build(T_TRUE, s["pts"])
    hyp = np.stack([s["near"], s["far"]])

    def neighbours():
        c = eng.cast_rays(s["t"], s["codes"], ow, dirv, normals=True, **RC)
        cs = eng.raycast_stats()
        a = eng.align_to_map(s["t"], s["codes"], s["pts"], hyp, per_point=True, iterations=3, trace=True, max_dist=MAX_DIST, huber=HUBER)
        as_ = eng.align_stats()
        q = eng.query_map(s["t"], s["codes"], pw, normals=True)
        out = [c[k].tobytes() for k in ("obj", "t", "dist", "status", "normal")] + [q[k].tobytes() for k in ("obj", "dist", "bound", "normal")]
        out += [np.ascontiguousarray(a[k]).tobytes() for k in ("pose", "cost", "information", "b", "obj", "dist")] + [repr(cs), repr(as_), repr(eng.query_stats())]
        return out
    before = neighbours()
    _align(eng, s, hyp, iterations=3)
    assert neighbours() == before


# ---- 11. edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges(eng):
    s = scene(eng)
    rho_gate = HUBER * (2.0 * MAX_DIST - HUBER)
    two = np.stack([s["near"], T_TRUE])
    # zero counts
    z = _align(eng, s, np.zeros((0, 4, 4)))
    assert z["pose"].shape == (0, 4, 4) and z["best"] == -1 and z["obj"].shape == (0, 300)
    for r in (_align(eng, s, two, pts=np.zeros((0, 3), F32)),
              eng.align_rays_to_map(np.zeros((0, 4, 4)), [], s["pts"], two, per_ray=True, max_gap=MAX_GAP, max_dist=MAX_DIST, huber=HUBER)):
        assert r["status"].tolist() == [L.ALIGN_NO_SUPPORT] * 2 and _same64(r["pose"], two) and r["best"] == -1
        assert np.all(r["cost"] == rho_gate) and np.all(r["obj"] == -1) and np.all(np.isposinf(r["dist"])) and not r["n_used"].any()
        assert np.all(np.isposinf(r["t"])) and np.all(r["status_ray"] == L.RAYCAST_MISS)
    assert eng.align_rays_stats()["evaluations"] == 0
    # all rays void (p_s == o_s): no support at the input pose, after one evaluation that marched nothing
    org = s["pts"].copy()
    r = _align(eng, s, s["near"][None], origins=org, iterations=4)
    assert r["status"][0] == L.ALIGN_NO_SUPPORT and _same64(r["pose"][0], s["near"]) and r["evaluations"][0] == 1 and r["n_used"][0] == 0
    assert np.all(r["obj"] == -1) and np.all(r["status_ray"] == L.RAYCAST_MISS) and r["cost"][0] == pytest.approx(rho_gate, rel=1e-12)
    st = eng.align_rays_stats()
    assert st["pairs"] == 0 and st["rows"] == 0 and st["evaluations"] == 1
    _record_is(r, 0, _ref_eval(eng, s, s["near"], org=org))
    # an object with a NaN code is never hit: its rays see through it
    codes = [c.copy() for c in s["codes"]]
    codes[1][5] = np.nan
    r = eng.align_rays_to_map(s["t"], codes, s["pts"], T_TRUE[None], per_ray=True, iterations=1, max_gap=MAX_GAP, raycast=RC, max_dist=MAX_DIST, huber=HUBER)
    assert not (r["obj"] == 1).any() and r["n_used"][0] == 200 and (r["obj"][0, 100:200] == -1).all()
    ev = AR.evaluate(T_TRUE, s["pts"], None, None, eng, A.Map(s["t"], codes), codes, HUBER, MAX_DIST, MAX_GAP, RC)
    _record_is(r, 0, ev)
    # origins given as zeros against NULL: the same bytes
    kw = dict(iterations=3, trace=True, weights=s["w"])
    assert _bytes(_align(eng, s, two, origins=np.zeros((300, 3), F32), **kw), trace=True) == _bytes(_align(eng, s, two, **kw), trace=True)
    # origins that are not the sensor's: the reference with them
    org = np.random.default_rng(12).uniform(-0.2, 0.2, (300, 3)).astype(F32)
    r = _align(eng, s, s["near"][None], origins=org, iterations=1)
    ev = _ref_eval(eng, s, s["near"], org=org)
    _record_is(r, 0, ev)
    _rays_are(r, 0, ev)
    # refusals, each with its message
    scaled = T_TRUE.copy()
    scaled[:3, :3] *= 1.01
    for bad, msg in ((dict(hyp=scaled[None]), "t_world_sensor0"), (dict(huber=0.4), "huber"), (dict(iterations=0), "iterations"), (dict(min_points=3), "min_points"),
                     (dict(weights=-np.ones(300, F32)), "weights"), (dict(max_gap=0.2), "max_gap"), (dict(max_gap=np.nan), "max_gap"),
                     (dict(raycast=dict(eps=0.0)), "eps"), (dict(raycast=dict(max_steps=5000)), "max_steps"), (dict(raycast=dict(relax=2.0)), "relax")):
        bad = dict(bad)
        hyp = bad.pop("hyp", T_TRUE[None])
        rc = bad.pop("raycast", RC)
        gap = bad.pop("max_gap", MAX_GAP)
        bad.setdefault("max_dist", MAX_DIST)
        bad.setdefault("huber", HUBER)
        with pytest.raises(L.DspError, match=r"\(-1\)") as err:
            eng.align_rays_to_map(s["t"], s["codes"], s["pts"], hyp, per_ray=True, max_gap=gap, raycast=rc, **bad)
        assert msg in str(err.value), (msg, str(err.value))
    # the cast's tables over all hypotheses' rays: 1024 objects x ceil(rows / 64) pair counts beyond 64 MiB
    many_t, many_c = np.repeat(s["t"][:1], 1024, 0), [s["codes"][0]] * 1024
    n = (64 << 20) // 4 // 1024 * 64 // 2 + 64
    with pytest.raises(L.DspError, match="split the request"):
        eng.align_rays_to_map(many_t, many_c, np.ones((n, 3), F32), two, max_gap=MAX_GAP, raycast=RC, iterations=1)
    # some per-ray outputs without the others
    lib = L.load()
    assert lib.dsp_map_align_rays(eng._h, None, None, 0, None, None, None, 0, None, 0, None, None, 1.0, None, None, None, None, None, None, None) == -1


# ---- 12. recovery ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start,iters", [("near", 8), ("mid", 12)])
def test_recovery(eng, start, iters):
    s = scene(eng)
    kw = dict(iterations=iters, trans_tol=0.0, rot_tol=0.0)
    res = _align(eng, s, s[start][None], **kw)
    ref = A.run(s[start], s["pts"], None, s["map"], None, evaluate=AR.evaluator(eng, s["codes"], None, MAX_GAP, RC), max_dist=MAX_DIST, huber=HUBER, **kw)
    pt = eng.align_to_map(s["t"], s["codes"], s["pts"], s[start][None], max_dist=MAX_DIST, huber=HUBER, **kw)
    dev_t, dev_r = A.pose_error(res["pose"][0], T_TRUE)
    ref_t, ref_r = A.pose_error(ref["pose"], T_TRUE)
    pt_t, pt_r = A.pose_error(pt["pose"][0], T_TRUE)
    print("ray recovery from %s: device %.3e / %.3e rad, reference loop %.3e / %.3e rad, point aligner %.3e / %.3e rad" % (
        start, dev_t, dev_r, ref_t, ref_r, pt_t, pt_r))
    parity_log(case="map_align_rays_recovery_" + start, dev_trans=dev_t, dev_rot=dev_r, ref_trans=ref_t, ref_rot=ref_r, point_trans=pt_t, point_rot=pt_r,
               cost=float(res["cost"][0]), n_used=int(res["n_used"][0]), point_cost=float(pt["cost"][0]), point_used=int(pt["n_used"][0]))
    assert dev_t <= 4 * ref_t and dev_r <= 4 * ref_r, (dev_t, ref_t, dev_r, ref_r)
