"""GPU: map alignment (include/dsp_gn.h dsp_map_align): batched SE(3) Gauss-Newton of a sensor-frame cloud against the map's surfaces.

The expected values come from tests/align_ref.py (pinned on the CPU by tests/test_align_host.py) composed with entry points that existed
before: tests/query_ref.py for containment and selection, Engine.sdf_jacobian rows per object at the reference's object-frame points.
Evaluations are compared bit for bit: the decoder rows are bit-identical across tile lists by the suite's own assertions, the float32
arithmetic is one rounding per operation on both sides, and the float64 sums follow one written tree.  Only exp_se3's sin / cos may differ
in the last place between the C library and Python, so a pose reached by a step is compared to 1e-14.
"""

import numpy as np
import pytest

import align_ref as A
import query_ref as Q
from conftest import parity_log
from dsp_slam_amd import engine as E, _lib as L

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MAX_DIST, HUBER = 0.3, 0.05
STEP = (1e-3, 4.0, 0.5, 1e-9, 1e6)


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


def _decoder(eng, codes):
    def decode(o, p):
        v, g = eng.sdf_jacobian(codes[o], p)
        return v, g[:, -3:]
    return decode


def _in_ball(rng, n, r=1.0):
    u = rng.normal(size=(n, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    return u * (r * rng.uniform(0, 1, (n, 1)) ** (1 / 3))


def _world(t, p_obj):
    return p_obj @ t[:3, :3].astype(F64).T + t[:3, 3].astype(F64)


def _to_sensor(T_true, world):
    inv = np.linalg.inv(T_true)
    return (world @ inv[:3, :3].T + inv[:3, 3]).astype(F32)


T_TRUE = A.rigid(A.axis_angle([0.3, -1.0, 0.5], 0.7), [0.5, -1.5, 2.0])
_SCENE, _SCENE2 = {}, {}


def scene(eng):
    """Three objects whose spheres do not overlap, 100 points per object on the decoded surface, in the sensor frame; the start poses;
    computed once, never modified."""
    if not _SCENE:
        rng = np.random.default_rng(7)
        t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [2.6, 0.3, -0.2], [4.0, -3.0, 1.0]])
        codes = list(rng.uniform(-0.3, 0.3, (3, 64)).astype(F32))
        start = [_in_ball(rng, 600, 0.5).astype(F32) for _ in range(3)]
        world = []
        start = [r["vertices"] for r in eng.surface_points(codes, start, steps=8)]           # 8 steps a call: two calls
        for o, r in enumerate(eng.surface_points(codes, start, steps=8)):
            p = r["vertices"].astype(F64)
            keep = p[(np.abs(r["sdf"]) < 1e-6) & (np.sqrt((p * p).sum(1)) < 0.9)][:100]
            assert keep.shape[0] == 100, (o, keep.shape)
            world.append(_world(t[o], keep))
        world = np.concatenate(world)
        centre = world.mean(0)
        near, far = A.offset_pose(rng, T_TRUE, 5.0, 0.05, centre), A.offset_pose(rng, T_TRUE, 30.0, 0.3, centre)
        mid = A.offset_pose(rng, T_TRUE, 20.0, 0.2, centre)
        w = rng.uniform(0.0, 2.0, 300).astype(F32)
        w[rng.permutation(300)[:20]] = 0.0
        _SCENE.update(t=t, codes=codes, map=A.Map(t, codes), decode=_decoder(eng, codes), pts=_to_sensor(T_TRUE, world), centre=centre, near=near, far=far,
                      mid=mid, w=w, rng=rng)
    return _SCENE


def scene2(eng):
    """The overlapping layout of tests/test_gpu_map_query.py (spheres 0 and 1 overlap, 120 of the 300 points in the overlap), seen from a
    sensor frame: winners change between chunks."""
    if not _SCENE2:
        rng = np.random.default_rng(41)
        t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [1.25, 0.3, -0.2], [4.0, -3.0, 1.0]])
        codes = list(np.random.default_rng(42).uniform(-0.3, 0.3, (3, 64)).astype(F32))
        lens = []
        while sum(len(x) for x in lens) < 120:
            cand = _world(t[0], _in_ball(rng, 400)).astype(F32)
            ins = Q.candidates(*Q.invert(t)[:2], cand)[1]
            lens.append(cand[ins[0] & ins[1]])
        lens = np.concatenate(lens)[:120]
        inside = np.concatenate([_world(t[o], _in_ball(rng, 35, 0.98)) for o in range(3)])
        outside = np.concatenate([_world(t[o], _in_ball(rng, 25, 1.0) * 1.7) for o in range(3)])
        world = np.concatenate([lens.astype(F64), inside, outside])
        assert world.shape == (300, 3)
        hyp = np.stack([T_TRUE, A.offset_pose(rng, T_TRUE, 2.0, 0.02, world.mean(0))])
        _SCENE2.update(t=t, codes=codes, map=A.Map(t, codes), decode=_decoder(eng, codes), pts=_to_sensor(T_TRUE, world), hyp=hyp)
    return _SCENE2


def _ref_eval(s, T, pts=None, w=None):
    return A.evaluate(T, s["pts"] if pts is None else pts, w, s["map"], s["decode"], HUBER, MAX_DIST)


def _align(eng, s, hyp, pts=None, weights=None, **kw):
    kw.setdefault("max_dist", MAX_DIST)
    kw.setdefault("huber", HUBER)
    return eng.align_to_map(s["t"], s["codes"], s["pts"] if pts is None else pts, hyp, weights=weights, per_point=True, **kw)


def _record_is(res, k, ev):
    """hypothesis k's returned record is the reference evaluation ev, bit for bit"""
    assert _same64(res["information"][k], A.full_h(ev["sums"])), k
    assert _same64(res["b"][k], ev["sums"][A.IDX_B:A.IDX_B + 6]), k
    assert _same64(res["cost"][k:k + 1], np.array([ev["cost"]])), (k, res["cost"][k], ev["cost"])
    assert res["n_used"][k] == ev["n_used"] and _same64(res["sum_w"][k:k + 1], ev["sums"][A.IDX_W:A.IDX_W + 1]), k


RESULT_KEYS = ("pose", "status", "evaluations", "steps", "cost0", "cost", "n_used", "sum_w", "lambda", "information", "b", "obj", "dist")


def _bytes(res, k=None, trace=False):
    """the bytes of a result, of hypothesis k or of all"""
    sl = slice(None) if k is None else slice(k, k + 1)
    out = [np.ascontiguousarray(res[key][sl]).tobytes() for key in RESULT_KEYS]
    if trace:
        out += [np.ascontiguousarray(res["trace"][key][sl]).tobytes() for key in sorted(res["trace"])]
    return out


# ---- 1. evaluate only --------------------------------------------------------------------------------------------------------------------
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
    assert res["evaluations"].tolist() == [1, 1, 1] and res["steps"].tolist() == [0, 0, 0]
    assert eng.align_stats()["evaluations"] == 1
    used = []
    for k in range(3):
        ev = _ref_eval(s, hyp[k], pts, w)
        _record_is(res, k, ev)
        assert np.array_equal(res["obj"][k], ev["obj"]) and _same32(res["dist"][k], ev["dist"]), k
        assert _same64(res["pose"][k], hyp[k]) and _same64(res["cost0"][k:k + 1], res["cost"][k:k + 1])
        assert res["status"][k] == (L.ALIGN_NO_SUPPORT if ev["n_used"] < 6 else L.ALIGN_OK)
        used.append(ev["n_used"])
    if n == 300:
        assert used[0] == (280 if weighted else 300) and used[1] == used[0] and used[2] < used[0]       # the scene: gate and support differ
        assert res["best"] == 0


# ---- 2. every evaluation of a run ---------------------------------------------------------------------------------------------------------
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
    res = _align(eng, s, hyp, iterations=12, trans_tol=0.0, rot_tol=0.0, trace=True, **kw)
    tr = res["trace"]
    for k in range(2):
        n_ev = int(res["evaluations"][k])
        assert n_ev == 12 and np.all(tr["decision"][k] != 0)
        assert _same64(tr["pose"][k, 0], hyp[k])
        acc = None
        for e in range(n_ev):
            ev = _ref_eval(s, tr["pose"][k, e])
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
        # the returned state is the last accepted one, with its record
        _record_is(res, k, acc)
        assert _same64(res["pose"][k], acc["pose"]) and res["steps"][k] == (tr["decision"][k, 1:] == A.ACCEPTED).sum()
        assert np.array_equal(res["obj"][k], acc["obj"]) and _same32(res["dist"][k], acc["dist"])
    if step_control:
        assert (tr["decision"] == A.REJECTED).any()        # at float32's floor the cost stops falling: the rule rejects, lambda grows
    et, er = A.pose_error(res["pose"][0], T_TRUE)
    assert et < 1e-4 and er < 1e-4, (et, er)


# ---- 3. recovery -------------------------------------------------------------------------------------------------------------------------
def test_recovery_from_five_degrees(eng):
    s = scene(eng)
    kw = dict(iterations=8, trans_tol=0.0, rot_tol=0.0)
    res = _align(eng, s, np.stack([s["near"], s["far"]]), **kw)
    ref = A.run(s["near"], s["pts"], None, s["map"], s["decode"], max_dist=MAX_DIST, huber=HUBER, **kw)
    dev_t, dev_r = A.pose_error(res["pose"][0], T_TRUE)
    ref_t, ref_r = A.pose_error(ref["pose"], T_TRUE)
    ratio = float(res["cost"][1] / res["cost"][0])
    print("recovery: device %.3e / %.3e rad, reference loop %.3e / %.3e rad; 30-degree hypothesis cost ratio %.3e" % (dev_t, dev_r, ref_t, ref_r, ratio))
    parity_log(case="map_align_recovery", dev_trans=dev_t, dev_rot=dev_r, ref_trans=ref_t, ref_rot=ref_r, far_cost_ratio=ratio,
               cost=float(res["cost"][0]), far_cost=float(res["cost"][1]), far_used=int(res["n_used"][1]))
    assert dev_t <= 4 * ref_t and dev_r <= 4 * ref_r, (dev_t, ref_t, dev_r, ref_r)
    assert res["best"] == 0 and res["n_used"][0] == 300


# ---- 4. independence and determinism ------------------------------------------------------------------------------------------------------
def test_hypotheses_are_independent_and_calls_repeat(eng):
    s = scene(eng)
    hyp = np.stack([s["near"], s["far"], s["mid"]])
    kw = dict(iterations=5, step_control=STEP, trace=True, weights=s["w"])
    whole = _align(eng, s, hyp, **kw)
    assert _bytes(whole, trace=True) == _bytes(_align(eng, s, hyp, **kw), trace=True)
    for k in range(3):
        assert _bytes(whole, k, trace=True) == _bytes(_align(eng, s, hyp[k:k + 1], **kw), trace=True), k


def test_more_chunks_return_the_same_bytes(eng):
    s = scene2(eng)
    lib = L.load()
    kw = dict(iterations=3, trace=True)
    whole = _align(eng, s, s["hyp"], **kw)
    st = eng.align_stats()
    assert lib.dsp_debug_query_chunk_rows(eng._h, 70) == 0
    try:
        chunked = _align(eng, s, s["hyp"], **kw)
        st2 = eng.align_stats()
    finally:
        assert lib.dsp_debug_query_chunk_rows(eng._h, 0) == 0
    assert _bytes(chunked, trace=True) == _bytes(whole, trace=True)
    assert st2["rows"] == st["rows"] and st2["chunks"] > 2 * st["chunks"] and st["chunks"] == st["evaluations"] == 3
    # the reference at the start poses: the overlap is decided by distance both ways, so a later chunk's winner wrote over an earlier one's gradient
    for k in range(2):
        ev = _ref_eval(s, s["hyp"][k])
        tr = chunked["trace"]
        assert _same64(tr["H"][k, 0], A.full_h(ev["sums"])) and _same64(tr["b"][k, 0], ev["sums"][A.IDX_B:A.IDX_B + 6]) and tr["n_used"][k, 0] == ev["n_used"]
        ins = Q.candidates(s["map"].rt, s["map"].s, ev["pw"])[1]
        both = ins[0] & ins[1]
        assert both.sum() >= 40 and set(np.unique(ev["obj"][both])) == {0, 1}


# ---- 5. ended hypotheses cost nothing -----------------------------------------------------------------------------------------------------
def test_an_ended_hypothesis_costs_no_rows(eng):
    """At T_true itself the first solved step is already float32 noise (measured: 5e-8, then 1e-7, 2e-7 -- it does not shrink), so with any
    tolerance a later step can meet, that hypothesis converges at its FIRST evaluation.  The hypothesis that converges at its second
    evaluation therefore starts 1e-4 off T_true: its first step is 1e-4, its second is noise.  Both are here, next to one that runs on."""
    s = scene(eng)
    close = A.offset_pose(np.random.default_rng(5), T_TRUE, 0.005, 1e-4, s["centre"])
    hyp = np.stack([T_TRUE, close, s["near"]])
    res = _align(eng, s, hyp, iterations=6, trace=True)                      # the default tolerances: 1e-6
    st = eng.align_stats()
    assert res["evaluations"][:2].tolist() == [1, 2] and res["status"][:2].tolist() == [L.ALIGN_CONVERGED] * 2 and res["evaluations"][2] > 2
    assert res["steps"][:2].tolist() == [0, 1]
    rows = 0
    for k in range(3):
        for e in range(int(res["evaluations"][k])):
            rows += int(Q.candidates(s["map"].rt, s["map"].s, A.transform(res["trace"]["pose"][k, e], s["pts"]))[1].sum())
    assert st["rows"] == rows and st["evaluations"] == int(res["evaluations"].max())
    for k in range(2):
        n_ev = int(res["evaluations"][k])
        assert not res["trace"]["decision"][k, n_ev:].any() and not res["trace"]["pose"][k, n_ev:].any()
        assert _bytes(res, k) == _bytes(_align(eng, s, hyp[k:k + 1], iterations=n_ev))


# ---- 6. pass border ----------------------------------------------------------------------------------------------------------------------
def test_rows_across_the_pass_border(eng):
    s = scene(eng)
    n = 66000
    rng = np.random.default_rng(6)
    pts = (rng.uniform(-1, 1, (n, 3)) + [1000.0, 1000.0, 1000.0]).astype(F32)       # far outside every sphere, under either hypothesis
    # rows are h n + i: row 65 536 is (h 0, i 65 536), row 131 072 is (h 1, i 65 072)
    idx = np.concatenate([np.arange(100), np.arange(65536 - 50, 65536 + 50), np.arange(131072 - n - 50, 131072 - n + 50)])
    assert np.unique(idx).size == 300
    pts[idx] = s["pts"][rng.permutation(300)]
    hyp = np.stack([s["near"], T_TRUE])
    res = _align(eng, s, hyp, pts=pts, iterations=1)
    st = eng.align_stats()
    assert st["passes"] >= 2 and st["evaluations"] == 1
    for k in range(2):
        ev = _ref_eval(s, hyp[k], pts)
        _record_is(res, k, ev)
        assert ev["n_used"] == 300 and np.array_equal(res["obj"][k], ev["obj"]) and _same32(res["dist"][k], ev["dist"])
    assert st["rows"] == 600


# ---- 7. edges ----------------------------------------------------------------------------------------------------------------------------
def test_edges(eng):
    s = scene(eng)
    rho_gate = HUBER * (2.0 * MAX_DIST - HUBER)
    # no point inside any sphere
    away = s["pts"] + F32(500.0)
    res = _align(eng, s, s["near"][None], pts=away, iterations=4)
    assert res["status"][0] == L.ALIGN_NO_SUPPORT and _same64(res["pose"][0], s["near"]) and res["n_used"][0] == 0 and res["evaluations"][0] == 1
    assert res["cost"][0] == pytest.approx(rho_gate, rel=1e-12) and np.all(res["obj"] == -1) and np.all(np.isposinf(res["dist"]))
    assert _same64(res["cost"][:1], np.array([_ref_eval(s, s["near"], away)["cost"]]))
    assert eng.align_stats()["rows"] == 0
    # NaN points and zero weights equal the call without those points -- in the result; the sums' tree depends on where the points sit, so
    # the points taken out are the LAST ones (a point inside the tree would shift its neighbours to other leaves)
    pts = np.concatenate([s["pts"], s["pts"][:40]])
    pts[300:320, 1] = np.nan
    w = np.ones(340, F32)
    w[320:] = 0.0
    a = _align(eng, s, s["near"][None], pts=pts, weights=w, iterations=4)
    b = _align(eng, s, s["near"][None], iterations=4)
    assert _bytes(a)[:-2] == _bytes(b)[:-2]
    assert np.array_equal(a["obj"][:, :300], b["obj"]) and np.all(a["obj"][0, 300:320] == -1) and np.all(a["obj"][0, 320:] >= 0)
    # zero counts
    z = _align(eng, s, np.zeros((0, 4, 4)))
    assert z["pose"].shape == (0, 4, 4) and z["best"] == -1
    for r in (_align(eng, s, np.stack([s["near"], T_TRUE]), pts=np.zeros((0, 3), F32)),
              eng.align_to_map(np.zeros((0, 4, 4)), [], s["pts"], np.stack([s["near"], T_TRUE]), per_point=True, max_dist=MAX_DIST, huber=HUBER)):
        assert r["status"].tolist() == [L.ALIGN_NO_SUPPORT] * 2 and _same64(r["pose"], np.stack([s["near"], T_TRUE])) and r["best"] == -1
        assert np.all(r["cost"] == rho_gate) and np.all(r["obj"] == -1) and np.all(np.isposinf(r["dist"])) and not r["n_used"].any()
    # refusals
    scaled = T_TRUE.copy()
    scaled[:3, :3] *= 1.01
    sheared = T_TRUE.copy()
    sheared[0, 1] += 0.05
    for bad in (dict(hyp=scaled[None]), dict(hyp=np.stack([T_TRUE, sheared])), dict(huber=0.4), dict(iterations=0), dict(min_points=3),
                dict(weights=-np.ones(300, F32))):
        hyp = bad.pop("hyp", T_TRUE[None])
        with pytest.raises(L.DspError, match=r"\(-1\)"):
            _align(eng, s, hyp, **bad)
    # an object with a non-finite code never wins
    codes = [c.copy() for c in s["codes"]]
    codes[1][5] = np.nan
    r = eng.align_to_map(s["t"], codes, s["pts"], T_TRUE[None], per_point=True, iterations=1, max_dist=MAX_DIST, huber=HUBER)
    assert not (r["obj"] == 1).any() and r["n_used"][0] == 200 and (r["obj"] == -1).sum() == 100
    ev = A.evaluate(T_TRUE, s["pts"], None, A.Map(s["t"], codes), s["decode"], HUBER, MAX_DIST)
    _record_is(r, 0, ev)


# ---- 8. coexistence ----------------------------------------------------------------------------------------------------------------------
def test_the_query_is_unchanged_around_an_align_call(eng):
    s = scene(eng)
    world = A.transform(T_TRUE, s["pts"])
    before = eng.query_map(s["t"], s["codes"], world, normals=True)
    st = eng.query_stats()
    _align(eng, s, np.stack([s["near"], s["far"]]), iterations=3)
    after = eng.query_map(s["t"], s["codes"], world, normals=True)
    assert all(before[k].tobytes() == after[k].tobytes() for k in ("obj", "dist", "bound", "normal")) and eng.query_stats() == st
    assert (before["obj"] >= 0).all()
