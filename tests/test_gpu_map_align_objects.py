"""GPU: object refinement (include/dsp_gn.h dsp_map_align_objects): one SE(3) correction per map object against world-frame depth rays from
known sensor poses, the Gauss-Newton sums segmented by the object a ray sees.

The expected values come from tests/align_objects_ref.py (pinned on the CPU by tests/test_align_objects_host.py) composed with what existed
before: tests/raycast_ref.py marches the rays through Engine.decode_sdf, Engine.sdf_jacobian gives the winners' rows at the restatement's
own hit samples, tests/align_rays_ref.py the residual and the match, tests/align_ref.py the rows, the tree, the step and the rule.
Evaluations are compared bit for bit; a correction reached by a step to 1e-14 (exp_se3's sin / cos).

The scenes are those of tests/test_gpu_map_align_rays.py, their sensor-frame observations moved to the world frame at the sensor's true
pose, and -- for the recovery -- the three-object layout of tests/test_align_objects_host.py seen from its two sensor positions.
"""
import ctypes as C

import numpy as np
import pytest

import align_objects_ref as AO
import align_rays_ref as AR
import align_ref as A
import test_align_objects_host as H
import test_gpu_early_stop as ES
import test_gpu_map_align_rays as TR
from conftest import parity_log
from dsp_slam_amd import engine as E, _lib as L
from test_align_rays_host import aimed_rays

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MAX_DIST, HUBER, MAX_GAP, RC, STEP = TR.MAX_DIST, TR.HUBER, TR.MAX_GAP, TR.RC, TR.STEP
_same32, _same64 = TR._same32, TR._same64


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


_WORLD, _WORLD2, _TWO = {}, {}, {}


def world(eng):
    """The segmented scene of the ray alignment's tests in the world frame: its 300 observations at T_TRUE (100 per object, in object
    order), the true map, and the map with every object displaced by its own offset (5, 12 and 20 degrees about its centre)."""
    if not _WORLD:
        s = TR.scene(eng)
        pw, ow, _ = AR.build(TR.T_TRUE, s["pts"])
        _WORLD.update(t=s["t"], codes=s["codes"], pw=pw, ow=ow, w=s["w"], t0=H.displaced(np.random.default_rng(21), s["t"]))
    return _WORLD


def world2(eng):
    """The occlusion scene (object 0 stands in front of object 1) in the world frame."""
    if not _WORLD2:
        s = TR.scene2(eng)
        pw, ow, _ = AR.build(s["T_true"], s["pts"])
        _WORLD2.update(t=s["t"], codes=s["codes"], pw=pw, ow=ow, seen=s["seen"], n_graze=s["n_graze"])
    return _WORLD2


def two_sensors(eng):
    """The recovery scene of tests/test_align_objects_host.py observed by the device: the three objects at their TRUE poses seen from both
    sensor positions by Engine.cast_rays (eps 1e-5, 256 steps), PER_OBJ hits per object and sensor; the displaced map."""
    if not _TWO:
        rng = np.random.default_rng(H.SEED)
        t_true, codes = H.layout(rng)
        codes = list(codes)
        pw, ow = [], []
        for T in H.SENSORS:
            dirs = aimed_rays(rng, t_true, T, 2 * H.PER_OBJ)
            pts, seen, _, _ = TR.observe(eng, t_true, codes, T, dirs, H.PER_OBJ)
            assert pts.shape == (3 * H.PER_OBJ, 3), pts.shape
            p, o = H.world_rays(pts, T)
            pw.append(p.astype(F32)); ow.append(o.astype(F32))
        _TWO.update(t_true=t_true, codes=codes, pw=np.concatenate(pw), ow=np.concatenate(ow), t0=H.displaced(rng, t_true))
    return _TWO


def _refine(eng, t, codes, pw, ow, **kw):
    kw.setdefault("max_dist", MAX_DIST)
    kw.setdefault("huber", HUBER)
    kw.setdefault("max_gap", MAX_GAP)
    kw.setdefault("raycast", RC)
    kw.setdefault("per_ray", True)
    return eng.align_objects_to_rays(t, codes, pw, ow, **kw)


def _ref_eval(eng, poses32, codes, pw, ow, w=None, max_gap=MAX_GAP, budget=None):
    return AO.evaluate(poses32, codes, pw, ow, w, eng, HUBER, MAX_DIST, max_gap, RC, budget)


def _record_is(res, k, sums):
    """object k's returned record holds these sums, bit for bit"""
    assert _same64(res["information"][k], A.full_h(sums)), k
    assert _same64(res["b"][k], sums[A.IDX_B:A.IDX_B + 6]), k
    assert _same64(res["cost"][k:k + 1], np.array([A.cost_of(sums, HUBER, MAX_DIST)])), (k, res["cost"][k])
    assert res["n_used"][k] == int(sums[A.IDX_N]) and _same64(res["sum_w"][k:k + 1], sums[A.IDX_W:A.IDX_W + 1]), k


def _rays_are(res, ev):
    assert np.array_equal(res["obj"], ev["obj"]) and _same32(res["dist"], ev["dist"])
    assert _same32(res["t"], ev["t"]) and np.array_equal(res["status_ray"], ev["status"])


RESULT_KEYS = ("t_world_obj", "correction", "status", "evaluations", "steps", "cost0", "cost", "n_used", "sum_w", "lambda", "information", "b", "obj", "dist",
               "t", "status_ray")


def _bytes(res, trace=False):
    out = [np.ascontiguousarray(res[key]).tobytes() for key in RESULT_KEYS]
    if trace:
        out += [np.ascontiguousarray(res["trace"][key]).tobytes() for key in sorted(res["trace"])]
    return out


def _object_error(T, T_true):
    """(distance between the objects' centres, rotation angle in radians) of pose T against T_true"""
    T, T_true = np.asarray(T, F64), np.asarray(T_true, F64)
    return float(np.sqrt(((T[:3, 3] - T_true[:3, 3]) ** 2).sum())), A.pose_error(T, T_true)[1]


# ---- 1. one evaluation, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_one_evaluation_is_the_reference_bit_for_bit(eng, n, weighted):
    s = world(eng)
    idx = np.arange(300) if n == 300 else np.sort(np.random.default_rng(n).permutation(300)[:n])
    pw, ow = s["pw"][idx], s["ow"][idx]
    w = s["w"][idx].copy() if weighted else None
    if weighted and n == 1:
        w[0] = 1.5
    for poses in (s["t"], s["t0"]):
        res = _refine(eng, poses, s["codes"], pw, ow, weights=w, iterations=1, trans_tol=0.0, rot_tol=0.0)
        ev = _ref_eval(eng, poses, s["codes"], pw, ow, w)
        st = eng.align_objects_stats()
        assert res["evaluations"].tolist() == [1, 1, 1] and res["steps"].tolist() == [0, 0, 0] and st["evaluations"] == 2     # one more for the rays
        for k in range(3):
            _record_is(res, k, ev["sums"][k])
            assert res["status"][k] == (L.ALIGN_NO_SUPPORT if ev["sums"][k, A.IDX_N] < 6 else L.ALIGN_OK)
            assert _same64(res["cost0"][k:k + 1], res["cost"][k:k + 1])
        _rays_are(res, ev)
        assert _same32(res["t_world_obj"], poses) and _same64(res["correction"], np.stack([np.eye(4)] * 3))
    if n == 300:
        at_true = _refine(eng, s["t"], s["codes"], pw, ow, weights=w, iterations=1)
        assert at_true["n_used"].sum() == (280 if weighted else 300)             # at the true map every ray sees what it measured


def test_two_tree_blocks_and_an_object_nobody_sees(eng):
    """600 rays: object 1's hundred rays four times over (400 winners: two blocks of the tree), and a fourth object far from every ray."""
    s = world(eng)
    idx = np.sort(np.concatenate([np.arange(300), np.tile(np.arange(100, 200), 3)]))
    pw, ow = s["pw"][idx], s["ow"][idx]
    w = np.random.default_rng(8).uniform(0.0, 2.0, 600).astype(F32)
    far = s["t0"][2].copy()
    far[:3, 3] += F32(40.0)
    poses, codes = np.concatenate([s["t0"], far[None]]), s["codes"] + [s["codes"][2]]
    res = _refine(eng, poses, codes, pw, ow, weights=w, iterations=1)
    ev = _ref_eval(eng, poses, codes, pw, ow, w)
    counts = [int((ev["winner"] == k).sum()) for k in range(4)]
    assert counts[1] > 256 and counts[3] == 0 and counts[0] > 0, counts
    for k in range(4):
        _record_is(res, k, ev["sums"][k])
    _rays_are(res, ev)
    assert res["status"][3] == L.ALIGN_NO_SUPPORT and res["n_used"][3] == 0 and res["sum_w"][3] == 0 and _same32(res["t_world_obj"][3], far)
    assert np.all(np.signbit(res["b"][3])) and not res["information"][3].any()


# ---- 2. every evaluation of a run --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step_control", [True, False])
def test_every_evaluation_of_a_run_is_the_reference(eng, step_control):
    s = world(eng)
    iters = 6
    kw = dict(step_control=STEP) if step_control else {}
    res = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], iterations=iters, trans_tol=0.0, rot_tol=0.0, trace=True, **kw)
    tr = res["trace"]
    assert res["evaluations"].tolist() == [iters] * 3 and np.all(tr["decision"] != 0) and _same64(tr["pose"][:, 0], np.stack([np.eye(4)] * 3))
    acc_C, acc_sums = [None] * 3, [None] * 3
    for e in range(iters):
        # every object is evaluated at every evaluation of this run: the map of evaluation e stands at the traced corrections
        poses = AO.compose_all(tr["pose"][:, e], s["t0"])
        ev = _ref_eval(eng, poses, s["codes"], s["pw"], s["ow"])
        for k in range(3):
            sums = ev["sums"][k]
            assert sums[A.IDX_N] >= 6                                          # the replay of the rule below assumes support throughout
            assert _same64(tr["H"][k, e], A.full_h(sums)) and _same64(tr["b"][k, e], sums[A.IDX_B:A.IDX_B + 6]), (k, e)
            assert _same64(tr["cost"][k, e:e + 1], np.array([A.cost_of(sums, HUBER, MAX_DIST)])) and tr["n_used"][k, e] == int(sums[A.IDX_N]), (k, e)
            if tr["decision"][k, e] == A.ACCEPTED:
                acc_C[k], acc_sums[k] = tr["pose"][k, e], sums
            xi = A.solve(A.full_h(acc_sums[k]), acc_sums[k][A.IDX_B:A.IDX_B + 6], 0.0, tr["lambda"][k, e])
            assert xi is not None and _same64(tr["xi"][k, e], xi), (k, e)
            if e + 1 < iters:
                nxt = A.apply_step(xi, acc_C[k])
                assert np.all(np.abs(tr["pose"][k, e + 1] - nxt) <= 1e-14 * np.maximum(1.0, np.abs(nxt))), (k, e)
    for k in range(3):
        if step_control:
            dec, lam = TR._step_rule(tr["cost"][k])
            assert np.array_equal(tr["decision"][k], dec) and _same64(tr["lambda"][k], lam), k
        else:
            assert np.all(tr["decision"][k] == A.ACCEPTED) and not tr["lambda"][k].any()
        _record_is(res, k, acc_sums[k])                                        # the returned state is the last accepted one
        assert _same64(res["correction"][k], acc_C[k]) and res["steps"][k] == (tr["decision"][k, 1:] == A.ACCEPTED).sum()
    returned = AO.compose_all(np.stack(acc_C), s["t0"])
    assert _same32(res["t_world_obj"], returned)
    _rays_are(res, _ref_eval(eng, returned, s["codes"], s["pw"], s["ow"]))           # the extra evaluation of the returned map
    assert eng.align_objects_stats()["evaluations"] == iters + 1


# ---- 3. occlusion ------------------------------------------------------------------------------------------------------------------------
def test_occlusion(eng):
    s = world2(eng)
    res = _refine(eng, s["t"], s["codes"], s["pw"], s["ow"], iterations=1)
    ev = _ref_eval(eng, s["t"], s["codes"], s["pw"], s["ow"])
    for k in range(2):
        _record_is(res, k, ev["sums"][k])
    _rays_are(res, ev)
    # rays that measured object 1 and see object 0 (the grazing rays of the scene): they are rows of object 0 -- the sums just compared hold
    # them there -- and the gap gate decides whether they are matched
    front = eng.cast_rays(s["t"], s["codes"], s["ow"], (s["pw"] - s["ow"]).astype(F32), **RC)
    assert np.array_equal(ev["winner"], front["obj"])
    occl = (s["seen"] == 1) & (ev["winner"] == 0)
    print("rays that measured object 1 and see object 0: %d (the scene looked for %d)" % (occl.sum(), s["n_graze"]))
    assert occl.sum() >= 1 and np.all((res["obj"][occl] == 0) | (res["obj"][occl] == -1))
    without = AO.rows(s["pw"][~occl], ev["winner"][~occl], ev["obj"][~occl], ev["dist"][~occl], ev["gw"][~occl], None, 2, HUBER, MAX_DIST)
    assert without[0, A.IDX_W] == ev["sums"][0, A.IDX_W] - occl.sum() and without[1, A.IDX_W] == ev["sums"][1, A.IDX_W]
    with np.errstate(all="ignore"):
        length = np.sqrt(((s["pw"] - s["ow"]).astype(F64) ** 2).sum(1))
        gated = np.abs(length - res["t"].astype(F64)) > MAX_GAP + 1e-5
    assert np.all(res["obj"][gated] == -1)
    assert res["n_used"][0] + res["n_used"][1] <= (res["obj"] >= 0).sum() and res["n_used"].min() >= 100
    # object 0 displaced, object 1 not refined: object 1 returns its input bytes, object 0 moves back.  This scene shows ONE side of object 0
    # from ONE position, and that side hardly changes when the object slides along it: H's smallest eigenvalue at the start is 2e-4 (a
    # pure translation), the next one 3.7, the largest 1e2 (the float64 loop on the CPU shows the same figures), and an undamped
    # Gauss-Newton step runs 2 units along the unobserved direction and loses every ray.  damp = 0.1 lies between the two eigenvalues: it
    # keeps the step out of the direction the rays do not see and leaves the five observed ones alone (profiles/map_align_objects.md).
    t0 = s["t"].copy()
    t0[0] = A.offset_pose(np.random.default_rng(6), s["t"][0].astype(F64), 5.0, 0.05, s["t"][0, :3, 3].astype(F64)).astype(F32)
    part = _refine(eng, t0, s["codes"], s["pw"], s["ow"], refine=[1, 0], iterations=6, trans_tol=0.0, rot_tol=0.0, damp=0.1)
    assert _same32(part["t_world_obj"][1], t0[1]) and part["evaluations"][1] == 0 and part["status"][1] == L.ALIGN_OK
    assert _same64(part["correction"][1], np.eye(4)) and not part["information"][1].any()
    before, after = _object_error(t0[0], s["t"][0]), _object_error(part["t_world_obj"][0], s["t"][0])
    print("object 0 in front of an unrefined object 1: %.3e / %.3e rad -> %.3e / %.3e rad" % (before + after))
    assert after[0] < before[0] and after[1] < before[1], (before, after)
    assert (part["obj"] == 1).sum() >= 100                                      # object 1 still stands in the map and is seen


# ---- 4. recovery -------------------------------------------------------------------------------------------------------------------------
def test_recovery(eng):
    s = two_sensors(eng)
    kw = dict(iterations=8, trans_tol=0.0, rot_tol=0.0)
    res = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], **kw)
    ref = AO.run(3, AO.evaluator(eng, s["t0"], s["codes"], s["pw"], s["ow"], None, HUBER, MAX_DIST, MAX_GAP, RC), max_dist=MAX_DIST, huber=HUBER, **kw)
    for k in range(3):
        start_t, start_r = A.pose_error(s["t0"][k].astype(F64), s["t_true"][k].astype(F64))
        dev_t, dev_r = A.pose_error(res["t_world_obj"][k].astype(F64), s["t_true"][k].astype(F64))
        ref_t, ref_r = A.pose_error(AO.compose(ref[k]["correction"], s["t0"][k]).astype(F64), s["t_true"][k].astype(F64))
        print("object %d from %.3e / %.3e rad: device %.3e / %.3e rad, reference loop %.3e / %.3e rad" % (k, start_t, start_r, dev_t, dev_r, ref_t, ref_r))
        parity_log(case="map_align_objects_recovery_%d" % k, dev_trans=dev_t, dev_rot=dev_r, ref_trans=ref_t, ref_rot=ref_r, start_trans=start_t,
                   start_rot=start_r, cost=float(res["cost"][k]), n_used=int(res["n_used"][k]))
        assert dev_t <= 4 * ref_t and dev_r <= 4 * ref_r, (k, dev_t, ref_t, dev_r, ref_r)


# ---- 5. same bytes, whatever the cut -----------------------------------------------------------------------------------------------------
def test_the_cut_the_repeat_and_the_batch_return_the_same_bytes(eng):
    s = world(eng)
    lib = L.load()
    kw = dict(iterations=3, trace=True, weights=s["w"], step_control=STEP)
    whole = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], **kw)
    st = eng.align_objects_stats()
    assert _bytes(whole, trace=True) == _bytes(_refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], **kw), trace=True)         # repeated
    assert st["evaluations"] == 4 and st["passes"] == 4
    for budget in (70, 257):           # rows per chunk: an object's ~100 winners cut across chunks, and chunks that end inside an object
        assert lib.dsp_debug_query_chunk_rows(eng._h, budget) == 0
        try:
            cut = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], **kw)
            st2 = eng.align_objects_stats()
        finally:
            assert lib.dsp_debug_query_chunk_rows(eng._h, 0) == 0
        assert _bytes(cut, trace=True) == _bytes(whole, trace=True), budget
        assert st2["pairs"] == st["pairs"] and st2["passes"] > st["passes"], budget
    # between two runs of a resident batch: the batch's results are unchanged around the call, and the call's by the batch
    prm = E.gn_params(num_iterations=10, lr=1.0)
    b = ES._batch(eng, ES._cold(), prm)
    try:
        rows = ES._rows(b)
        between = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], **kw)
        assert ES._same(ES._rows(b), rows)
    finally:
        b.close()
    assert _bytes(between, trace=True) == _bytes(whole, trace=True)


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------------
def test_edges(eng):
    s = world(eng)
    rho_gate = HUBER * (2.0 * MAX_DIST - HUBER)
    keep = [x.copy() for x in (s["t0"], s["pw"], s["ow"], s["w"])] + [c.copy() for c in s["codes"]]
    # no objects, no rays: no device, NO_SUPPORT with the input poses
    z = _refine(eng, np.zeros((0, 4, 4)), [], s["pw"], s["ow"])
    assert z["t_world_obj"].shape == (0, 4, 4) and z["correction"].shape == (0, 4, 4) and np.all(z["obj"] == -1) and np.all(np.isposinf(z["dist"]))
    assert np.all(np.isposinf(z["t"])) and np.all(z["status_ray"] == L.RAYCAST_MISS) and eng.align_objects_stats()["evaluations"] == 0
    r = _refine(eng, s["t0"], s["codes"], np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    assert r["status"].tolist() == [L.ALIGN_NO_SUPPORT] * 3 and _same32(r["t_world_obj"], s["t0"]) and _same64(r["correction"], np.stack([np.eye(4)] * 3))
    assert np.all(r["cost"] == rho_gate) and not r["n_used"].any() and not r["evaluations"].any() and r["obj"].shape == (0,)
    st = eng.align_objects_stats()
    assert st["evaluations"] == 0 and st["pairs"] == 0
    # fewer than min_points used rays: NO_SUPPORT and the input pose bytes, while the neighbours run on
    idx = np.concatenate([np.arange(0, 4), np.arange(100, 300)])
    r = _refine(eng, s["t0"], s["codes"], s["pw"][idx], s["ow"][idx], iterations=4)
    assert r["status"][0] == L.ALIGN_NO_SUPPORT and r["evaluations"][0] == 1 and r["n_used"][0] < 6 and _same32(r["t_world_obj"][0], s["t0"][0])
    assert _same64(r["correction"][0], np.eye(4)) and r["evaluations"][1] > 1 and not _same32(r["t_world_obj"][1], s["t0"][1])
    # void rays and NaN end points are absent: the sums of the call without them
    pw, ow = np.concatenate([s["pw"], s["ow"][:3], s["pw"][:3]]), np.concatenate([s["ow"], s["ow"][:3], s["ow"][:3]])
    pw[303:, 1] = np.nan
    plain = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], iterations=1)
    more = _refine(eng, s["t0"], s["codes"], pw, ow, iterations=1)
    for key in ("information", "b", "cost", "sum_w", "n_used"):
        assert np.ascontiguousarray(more[key]).tobytes() == np.ascontiguousarray(plain[key]).tobytes(), key
    assert np.all(more["obj"][300:] == -1) and np.all(more["status_ray"][300:] == L.RAYCAST_MISS) and np.all(np.isposinf(more["dist"][300:]))
    # refine all zero: the input map, nothing evaluated; the per-ray outputs are the returned (= input) map's
    r = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], refine=[0, 0, 0], iterations=5)
    assert _same32(r["t_world_obj"], s["t0"]) and not r["evaluations"].any() and r["status"].tolist() == [L.ALIGN_OK] * 3
    assert eng.align_objects_stats()["evaluations"] == 1 and np.array_equal(r["obj"], plain["obj"]) and _same32(r["dist"], plain["dist"])
    r = _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], refine=[0, 0, 0], iterations=5, per_ray=False)
    st = eng.align_objects_stats()
    assert _same32(r["t_world_obj"], s["t0"]) and st["evaluations"] == 0 and st["rows"] == 0 and "obj" not in r
    # an object with a NaN code is never hit and never supported; its rays see through it
    codes = [c.copy() for c in s["codes"]]
    codes[1][5] = np.nan
    r = _refine(eng, s["t"], codes, s["pw"], s["ow"], iterations=1)
    assert not (r["obj"] == 1).any() and r["status"][1] == L.ALIGN_NO_SUPPORT and r["n_used"].tolist() == [100, 0, 100]
    # refusals: every DSP_E_ARG of the check hook is refused by the call, each with its message
    for bad, msg in ((dict(huber=0.4), "huber"), (dict(iterations=0), "iterations"), (dict(min_points=3), "min_points"),
                     (dict(weights=-np.ones(300, F32)), "weights"), (dict(weights=np.full(300, np.nan, F32)), "weights"), (dict(max_gap=0.2), "max_gap"),
                     (dict(max_gap=np.nan), "max_gap"), (dict(raycast=dict(eps=0.0)), "eps"), (dict(raycast=dict(max_steps=5000)), "max_steps"),
                     (dict(raycast=dict(relax=2.0)), "relax"), (dict(step_control=(1e-3, 0.0, 0.0, 0.0, 0.0)), "")):
        with pytest.raises(L.DspError, match=r"\(-1\)") as err:
            _refine(eng, s["t0"], s["codes"], s["pw"], s["ow"], **bad)
        assert msg in str(err.value), (msg, str(err.value))
    with pytest.raises(L.DspError, match="origins_world"):
        _refine(eng, s["t0"], s["codes"], s["pw"], None)
    scaled = s["t0"].copy()
    scaled[1, :3, 0] *= F32(1.01)
    with pytest.raises(L.DspError, match="t_world_obj"):
        _refine(eng, scaled, s["codes"], s["pw"], s["ow"])
    many_t, many_c = np.repeat(s["t"][:1], 1024, 0), [s["codes"][0]] * 1024
    n = (64 << 20) // 4 // 1024 * 64 + 64
    with pytest.raises(L.DspError, match="split the request"):
        _refine(eng, many_t, many_c, np.ones((n, 3), F32), np.zeros((n, 3), F32), iterations=1, per_ray=False)
    lib = L.load()
    one = np.zeros(1, np.int32)         # some per-ray outputs without the others
    prm, rprm = eng.align_params(), eng.raycast_params()
    assert lib.dsp_map_align_objects(eng._h, None, None, 0, None, None, None, 0, None, C.byref(prm), C.byref(rprm), 1.0, None, None, None, None, None, None, None,
                                     None) == 0
    assert lib.dsp_map_align_objects(eng._h, None, None, 0, None, None, None, 0, None, C.byref(prm), C.byref(rprm), 1.0, None, None, None, L.ptr(one, L.c_i32p),
                                     None, None, None, None) == -1
    # the input arrays are not written
    for a, b in zip(keep, [s["t0"], s["pw"], s["ow"], s["w"]] + list(s["codes"])):
        assert a.tobytes() == b.tobytes()
