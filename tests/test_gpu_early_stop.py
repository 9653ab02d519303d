"""GPU: the per-object convergence rule (dsp_batch_convergence / dsp_batch_iterations_used, include/dsp_gn.h).

Objects are independent and a ragged batch equals its objects run alone, so the feature is tested EXACTLY: an object the rule stops after n
updates must return, bit for bit, what a fixed n-iteration run of the same batch returns for it -- pose, code, loss and status.  Nothing
here has a tolerance on results.  The iteration counts are predicted from a traced, unstopped run with the numpy statement of the rule
(tests/early_stop_rule.py); the tolerances are geometric means of two consecutive step norms of one object of that trace, and the tests
assert -- as a condition on their inputs -- that no step of any object lies within a factor FAR of a tolerance.

The batch: three cold objects (160 surface points + 200 rays, synth.make_object) and the same three warm-started from their own
10-iteration results.
"""
import numpy as np
import pytest

import early_stop_rule as R
from conftest import golden
from dsp_slam_amd import _lib as L, engine as E, synth

pytestmark = pytest.mark.gpu
INF = float("inf")
N_IT = 10
# Every step norm is at least this factor away from the tolerance it is compared with.  The device compares the fp64 step; the prediction
# reads it from the trace, which holds dx rounded to fp32 (relative 2^-24 = 6e-8): a factor of 1.001 is four orders of magnitude above that.
FAR = 1.001
COUNTERS = ("n_fwd_points", "n_jac_points", "n_insphere_points", "n_render_rows", "n_prepass_points")


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _batch(eng, objs, prm, trace=False):
    return eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                     [o.get("code0", np.zeros(64, np.float32)) for o in objs], trace=trace)


def _rows(b):
    b.run()
    return b.results()


def _same(a, b, sel=None):
    sel = slice(None) if sel is None else sel
    return all(np.array_equal(x[sel], y[sel], equal_nan=True) for x, y in zip(a, b))


def _steps(b, n_it, lr, pose_only=False):
    """(dx (n_it, n, u), pose step norms (n_it, n), code step norms (n_it, n)) of the traced run b has just made."""
    dx = np.stack([b.trace(e)["dx"] for e in range(n_it)]).astype(np.float64)
    f = 1.0 if pose_only else float(np.float32(lr))
    p = 6 if pose_only else 7
    sp = np.abs(f * dx[:, :, :p]).max(-1)
    sc = np.abs(f * dx[:, :, p:]).max(-1) if not pose_only else np.zeros_like(sp)
    return dx, sp, sc


def _far(steps, tol):
    return bool(np.all((steps > tol * FAR) | (steps < tol / FAR)))


def _predict(dx, lr, tp, tc, min_it=1, **kw):
    return np.array([R.n_used(dx[:, i], lr, tp, tc, min_it, **kw) for i in range(dx.shape[1])], np.int32)


def _pick(dx, sp, sc, lr, want):
    """Tolerances (pose, code), each the geometric mean of the step norms of two consecutive iterations of one object: the first pair that
    is FAR from every step of every object and whose predicted counts satisfy `want`."""
    def cands(s):
        out = [float(np.sqrt(s[e, i] * s[e + 1, i])) for i in range(s.shape[1]) for e in range(s.shape[0] - 1)]
        return [t for t in out if t > 0 and _far(s, t)]
    for tp in cands(sp):
        for tc in cands(sc):
            if want(_predict(dx, lr, tp, tc), _predict(dx, lr, tp, INF), _predict(dx, lr, INF, tc)):
                return tp, tc
    return None


def _mixed_enough(n):
    return len(set(n.tolist())) >= 3 and 10 in n and n.min() <= 2


def _cold():
    # two ordinary detections and one with a poor initial estimate (it is still moving after ten iterations)
    return [synth.make_object(300, n_surface=160, n_background=40), synth.make_object(301, n_surface=160, n_background=40),
            synth.make_object(302, n_surface=160, n_background=40, t_noise=0.6, yaw_noise_deg=15.0)]


def _warm_from(eng, cold, prm):
    b = _batch(eng, cold, prm)
    t, code, _, status = _rows(b)
    b.close()
    assert (status == 0).all()
    return [dict(o, t_cam_obj_init=t[i].copy(), code0=L.code64(code[i])) for i, o in enumerate(cold)]


class Mixed(object):
    """The six-object batch, its traced unstopped run and the tolerances picked from that trace (computed once per learning rate)."""

    def __init__(self, eng, lr):
        self.prm = E.gn_params(num_iterations=N_IT, lr=lr)
        self.lr = lr
        cold = _cold()
        self.objs = cold + _warm_from(eng, cold, self.prm)
        b = _batch(eng, self.objs, self.prm, trace=True)
        self.ref = _rows(b)
        self.ref_used = b.iterations_used()
        self.ref_stats = b.stats()
        self.dx, self.sp, self.sc = _steps(b, N_IT, lr)
        b.close()
        print("lr", lr, "pose steps\n", self.sp, "\ncode steps\n", self.sc)
        assert (self.ref[3] == 0).all() and np.isfinite(self.dx).all()
        self.tol = _pick(self.dx, self.sp, self.sc, lr, lambda both, p, c: _mixed_enough(both))
        assert self.tol is not None, "no tolerance pair gives three distinct counts with a 10 and a count <= 2 on this batch"
        print("tolerances", self.tol, "predicted", _predict(self.dx, lr, *self.tol))


@pytest.fixture(scope="module")
def mixed(eng):
    return Mixed(eng, 1.0)


def test_off_is_the_parent(eng, mixed):
    rows = {}
    for name, rule in (("none", None), ("zero", (0.0, 0.0, 1)), ("inf", (INF, INF, N_IT + 1))):
        b = _batch(eng, mixed.objs, mixed.prm)
        if rule:
            b.set_convergence(*rule)
        rows[name] = _rows(b)
        assert (b.iterations_used()[rows[name][3] == 0] == N_IT).all() and (rows[name][3] == 0).all()
        b.close()
    assert _same(rows["none"], mixed.ref) and _same(rows["zero"], rows["none"]) and _same(rows["inf"], rows["none"])


def _cases(m):
    tp, tc = m.tol
    return [("pose", (tp, INF, 1)), ("code", (INF, tc, 1)), ("both", (tp, tc, 1)), ("min4", (tp, tc, 4))]


def _rule_and_exactness(eng, m, cases):
    b = _batch(eng, m.objs, m.prm)
    fixed = {}
    for name, (tp, tc, mi) in cases:
        want = _predict(m.dx, m.lr, tp, tc, mi)
        b.set_iterations(N_IT)
        b.set_convergence(tp, tc, mi)
        got_rows = _rows(b)
        used = b.iterations_used()
        st = b.stats()
        print(name, "tolerances", (tp, tc, mi), "predicted", want, "used", used)
        assert np.array_equal(used, want), (name, used, want)
        assert (got_rows[3] == 0).all()
        if name == "both":
            assert _mixed_enough(used), used
        if used.min() < N_IT:          # frozen means free: fewer points than the unstopped run decoded
            for k in COUNTERS:
                assert st[k] < m.ref_stats[k] or (m.ref_stats[k] == 0 and st[k] == 0), (name, k, st[k], m.ref_stats[k])
        b.set_convergence(0.0, 0.0, 1)
        for n in sorted(set(used.tolist())):       # exactness: the objects stopped after n updates against the fixed n-iteration run
            if n not in fixed:
                b.set_iterations(n)
                fixed[n] = _rows(b)
                assert (b.iterations_used() == n).all()
            assert _same(got_rows, fixed[n], used == n), (name, n)
    b.close()


def test_rule_and_exactness(eng, mixed):
    _rule_and_exactness(eng, mixed, _cases(mixed))


def test_rule_and_exactness_at_half_the_learning_rate(eng):
    m = Mixed(eng, 0.5)
    tp, tc = m.tol
    _rule_and_exactness(eng, m, [("both", (tp, tc, 1))])


def test_frozen_means_free(eng, mixed):
    """Two copies of one cold object stop at the same n: every work counter equals the fixed n-iteration run's (prepass guard off on both
    sides: its per-launch sample would enter the counts)."""
    tp, tc = mixed.tol
    pred = _predict(mixed.dx, 1.0, tp, tc)
    i = next((i for i in range(6) if 1 < pred[i] < N_IT), int(np.argmin(pred)))
    objs = [mixed.objs[i], mixed.objs[i]]
    b = _batch(eng, objs, mixed.prm)
    b.set_prepass_guard(False)
    b.set_convergence(tp, tc)
    rows = _rows(b)
    used, st = b.iterations_used(), b.stats()
    n = int(used[0])
    assert used[1] == n and 1 <= n < N_IT, used
    b.set_convergence(0.0, 0.0, 1)
    b.set_iterations(n)
    rows_n = _rows(b)
    st_n = b.stats()
    b.close()
    assert _same(rows, rows_n)
    for k in COUNTERS:
        assert st[k] == st_n[k], (k, st[k], st_n[k])
    assert st["n_jac_points"] > 0 and st["n_insphere_points"] > 0


def _exact(b, tol, n_it=N_IT, need_stop=True):
    """Test 3 on batch b as it is configured: rows of the objects the rule stopped after n updates == the fixed n-iteration run's."""
    b.set_iterations(n_it)
    b.set_convergence(*tol)
    rows = _rows(b)
    used = b.iterations_used()
    b.set_convergence(0.0, 0.0, 1)
    for n in sorted(set(used.tolist())):
        b.set_iterations(n)
        assert _same(rows, _rows(b), used == n), (n, used)
    if need_stop:
        assert used.min() < n_it, used
    return rows, used


FORMS = {
    "wave": lambda b: b.set_wave_bookkeeping(1),
    "block": lambda b: b.set_wave_bookkeeping(0),
    "prepass_off": lambda b: b.set_prepass(L.PREPASS_OFF),
    "mask_reuse_on": lambda b: b.set_mask_reuse(1),
    "mask_reuse_off": lambda b: b.set_mask_reuse(0),
    "f16_compute": lambda b: (b.set_compute(L.COMPUTE_F16), b.set_lp_small_batches(1)),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_form(eng, mixed, form):
    b = _batch(eng, mixed.objs, mixed.prm)
    FORMS[form](b)
    rows, used = _exact(b, mixed.tol)
    b.close()
    print(form, "used", used)
    if form != "f16_compute":           # the forms are bit-identical: the stopped batch is the automatic plan's
        bb = _batch(eng, mixed.objs, mixed.prm)
        bb.set_convergence(*mixed.tol)
        assert _same(rows, _rows(bb)) and np.array_equal(used, bb.iterations_used())
        bb.close()


def test_detection_sized_object(eng, mixed):
    """One object of SLAM's own size (250 points, 450 rays): cluster + latency form, direct tiles, speculative band."""
    o = synth.make_object(310, n_surface=250, n_background=200)
    b = _batch(eng, [o], mixed.prm, trace=True)
    b.run()
    dx, sp, sc = _steps(b, N_IT, 1.0)
    tol = _pick(dx, sp, sc, 1.0, lambda both, p, c: 1 < both[0] < N_IT)
    assert tol is not None
    rows, used = _exact(b, tol)
    assert np.array_equal(used, _predict(dx, 1.0, *tol))
    b.close()
    # trace rows of the iterations a frozen object did not run are zeros
    b = _batch(eng, [o], mixed.prm, trace=True)
    b.set_convergence(*tol)
    b.run()
    n = int(b.iterations_used()[0])
    tr = b.trace(n)
    assert not tr["H"].any() and not tr["dx"].any() and tr["V"][0] == 0 and tr["m"][0] == 0 and tr["K"][0] == 0
    assert b.trace(n - 1)["H"].any()
    b.close()


def test_pose_only(eng):
    """The 8-iteration golden's object, a clean object and the clean object restarted from its own 8-iteration result (it stops before the
    inlier filter of iteration 4 and keeps all its points): each bit-identical to its fixed-n run."""
    g, g5 = golden("golden_pose_only_8it.npz"), golden("golden_pose_only.npz")
    objs = [(g["t_co_se3"], float(g["scale"]), g["pts"], g["code"]), (g5["t_co_se3"], float(g5["scale"]), g5["pts"][:200], g5["code"])]
    prm = E.gn_params(pose_only_iterations=8)

    def make(objs, trace=False):
        return eng.pose_batch(prm, [o[0] for o in objs], [o[1] for o in objs], [o[2] for o in objs], [o[3] for o in objs], trace=trace)
    b = make(objs[1:])
    b.run()
    t8 = b.results()[0]
    b.close()
    objs.append((t8[0].copy(), objs[1][1], objs[1][2], objs[1][3]))
    b = make(objs, trace=True)
    ref = _rows(b)
    assert (b.iterations_used()[ref[3] == 0] == 8).all()
    dx, sp, _ = _steps(b, 8, 1.0, pose_only=True)
    print("pose-only steps\n", sp)
    tol = None
    for i in range(3):
        for e in range(7):
            tp = float(np.sqrt(sp[e, i] * sp[e + 1, i]))
            n = _predict(dx, 1.0, tp, 0.0, n_pose=6, pose_only=True)
            if tp > 0 and _far(sp, tp) and n[2] <= 4 and n.max() > 5:
                tol = tp
                break
        if tol:
            break
    assert tol is not None, "no tolerance stops the restarted object before iteration 5 and leaves another object running past it"
    want = _predict(dx, 1.0, tol, 0.0, n_pose=6, pose_only=True)
    rows, used = _exact(b, (tol, 123.0), n_it=8)          # code_tol is ignored
    b.close()
    print("pose-only tolerance", tol, "predicted", want, "used", used)
    assert np.array_equal(used, want) and used[2] <= 4
    # through the one-shot front: a resident batch created and destroyed inside the call
    t = eng.estimate_pose_batch(prm, [o[0] for o in objs], [o[1] for o in objs], [o[2] for o in objs], [o[3] for o in objs], convergence=(tol, 0.0))
    assert np.array_equal(t, rows[0], equal_nan=True)


def _views(o):
    return [dict(t_ref_cam=np.eye(4, dtype=np.float32), pts=o["pts"], rays=o["rays"], depth=o["depth"])]


def test_multiview(eng, mixed):
    prm = mixed.prm
    # a one-view group with tolerances == the single-view batch with the same tolerances
    b = _batch(eng, mixed.objs, prm)
    b.set_convergence(*mixed.tol)
    single = _rows(b)
    single_used = b.iterations_used()
    b.close()
    mv = eng.multiview_batch(prm, [o["t_cam_obj_init"] for o in mixed.objs], [_views(o) for o in mixed.objs], [o.get("code0", np.zeros(64, np.float32)) for o in mixed.objs])
    mv.set_convergence(*mixed.tol)
    assert _same(_rows(mv), single) and np.array_equal(mv.iterations_used(), single_used)
    mv.close()
    # a ragged batch: a three-view object, a one-view object, a two-view object, and the three-view object warm-started from its own result
    o3, o2 = synth.make_object_multiview(21, n_views=3, n_surface=120, n_background=40), synth.make_object_multiview(22, n_views=2, n_surface=120, n_background=40)
    o1 = mixed.objs[0]
    t0, views = [o3["t_cam_obj_init"], o1["t_cam_obj_init"], o2["t_cam_obj_init"]], [o3["views"], _views(o1), o2["views"]]
    zero = np.zeros(64, np.float32)
    mv = eng.multiview_batch(prm, t0, views, [zero] * 3)
    t, code, _, status = _rows(mv)
    mv.close()
    assert (status == 0).all()
    t0.append(t[0].copy())
    views.append(o3["views"])
    codes = [zero] * 3 + [L.code64(code[0])]
    mv = eng.multiview_batch(prm, t0, views, codes, trace=True)
    mv.run()
    dx, sp, sc = _steps(mv, N_IT, 1.0)
    tol = _pick(dx, sp, sc, 1.0, lambda both, p, c: len(set(both.tolist())) >= 2 and both[3] < both[0] and both.min() < N_IT)
    assert tol is not None
    want = _predict(dx, 1.0, *tol)
    rows, used = _exact(mv, tol)
    print("multi-view tolerances", tol, "predicted", want, "used", used)
    assert used.shape == (4,) and np.array_equal(used, want)          # per object, not per view; the group stops as one
    # every member froze with its leader: the views of a stopped object produce no rows after it stopped
    mv.set_iterations(N_IT)
    mv.set_convergence(*tol)
    mv.run()
    for i, off in ((0, 0), (3, 6)):
        n = int(mv.iterations_used()[i])
        if n < N_IT:
            tv = mv.trace_views(n)
            assert not tv["K"][off:off + 3].any() and not tv["V"][off:off + 3].any()
            assert mv.trace_views(n - 1)["K"][off:off + 3].any()
    mv.close()
    # the Engine's one-shot front with the argument: a resident batch inside the call
    assert _same(eng.reconstruct_multiview_batch(prm, t0, views, codes, convergence=tol), rows)


def test_failures_stay_local(eng, mixed):
    bad_nan = dict(mixed.objs[0], pts=mixed.objs[0]["pts"].copy())
    bad_nan["pts"][5, 1] = np.nan
    bad_few = dict(mixed.objs[1], rays=np.full_like(mixed.objs[1]["rays"], np.nan))
    objs = [mixed.objs[0], bad_nan, mixed.objs[3], bad_few, mixed.objs[2], mixed.objs[4]]
    keep = [0, 2, 4, 5]
    out = {}
    for name, rule in (("off", None), ("on", mixed.tol)):
        b = _batch(eng, objs, mixed.prm)
        if rule:
            b.set_convergence(*rule)
        out[name] = (_rows(b), b.iterations_used())
        b.close()
    (rows_off, used_off), (rows_on, used_on) = out["off"], out["on"]
    assert rows_on[3][1] == rows_off[3][1] == L.OBJ_NAN and rows_on[3][3] == rows_off[3][3] == L.OBJ_FEW_SAMPLES
    assert (rows_on[3][keep] == 0).all()
    # updates applied before the failure: none -- with and without the rule
    assert used_on[1] == used_off[1] == 0 and used_on[3] == used_off[3] == 0
    assert (used_off[keep] == N_IT).all()
    b = _batch(eng, [objs[i] for i in keep], mixed.prm)
    b.set_convergence(*mixed.tol)
    alone = _rows(b)
    assert np.array_equal(b.iterations_used(), used_on[keep]) and used_on[keep].min() < N_IT
    b.close()
    assert _same([r[keep] for r in rows_on], alone)


def test_guard_rerun(oracle_decoder, mixed):
    """A forced bf16 margin of 2e-5 trips the guard (tests/test_gpu_prepass.py): the tripped objects run again with the prepass off AND the
    same rule, so rows and iteration counts are those of the prepass-off run with the same tolerances."""
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    out = {}
    for name, mode, delta in (("off", L.PREPASS_OFF, -1.0), ("trip", L.PREPASS_BF16, 2e-5)):
        b = _batch(own, mixed.objs, mixed.prm)
        b.set_prepass(mode, delta)
        b.set_convergence(*mixed.tol)
        out[name] = (_rows(b), b.iterations_used(), b.stats())
        b.close()
    own.close()
    assert out["trip"][2]["prepass_guard_rerun"] == 1 and out["trip"][2]["prepass_guard_trips"] > 0
    assert _same(out["trip"][0], out["off"][0]) and np.array_equal(out["trip"][1], out["off"][1])
    assert out["off"][1].min() < N_IT


def test_refused_arguments(eng, mixed):
    b = _batch(eng, mixed.objs[:2] + mixed.objs[3:4], mixed.prm)
    lib = L.load()
    assert lib.dsp_batch_iterations_used(b._h, L.ptr(np.zeros(3, np.int32), L.c_i32p)) == -4          # DSP_E_STATE: not run yet
    b.set_convergence(*mixed.tol)
    rows = _rows(b)
    used = b.iterations_used()
    assert used.min() < N_IT
    for bad in ((-1e-3, 1e-3, 1), (1e-3, -1e-3, 1), (float("nan"), 1e-3, 1), (1e-3, float("nan"), 1), (1e-3, 1e-3, 0), (1e-3, 1e-3, -2), (-INF, 1e-3, 1)):
        assert lib.dsp_batch_convergence(b._h, *bad) == -1, bad                                  # DSP_E_ARG
        with pytest.raises(L.DspError):
            b.set_convergence(*bad)
    assert lib.dsp_batch_iterations_used(b._h, None) == -1
    assert _same(_rows(b), rows) and np.array_equal(b.iterations_used(), used)                      # the previous rule is still in force
    b.close()
    # the one-shot front of a joint batch
    o = mixed.objs
    got = eng.reconstruct_batch(mixed.prm, [x["t_cam_obj_init"] for x in o[:2] + o[3:4]], [x["pts"] for x in o[:2] + o[3:4]], [x["rays"] for x in o[:2] + o[3:4]],
                                [x["depth"] for x in o[:2] + o[3:4]], [x.get("code0", np.zeros(64, np.float32)) for x in o[:2] + o[3:4]], convergence=mixed.tol)
    assert _same(got, rows)
