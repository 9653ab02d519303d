"""GPU: per-observation weights (dsp_batch_observation_weights, include/dsp_gn.h) through every layer.

  1. unit weights are the plain run bit for bit (joint, pose-only with the inlier filter, multi-view), and so is a batch whose weights were
     cleared again;
  2. a ray of weight 0 is absent: the run equals, bit for bit, the run of the batch built without those rays (50 and 64 depth samples; one
     latency-sized object, one three-object batch);
  3. weighted systems against the weighted fp64 reference (tests/weights_ref.py) at the device's own traced states on the device's own sets,
     every iteration through gn_metric.check_against_fp64 with TAU_H / TAU_B / TAU_SOLVE as they stand (no jitter allowance is claimed:
     pair=None) -- joint (40 / 513 / 2100 points, 30 / 450 rays), pose-only at 8 iterations, a ragged multi-view batch with an all-zero view;
  4. points of weight 0 equal removal within that metric; V and K equal;
  5. degenerate sums and errors;
  6. with the report, the posterior (MEAN and SUM), step control, the prior and the convergence rule, a partial re-run after a forced
     prepass-guard trip, and the f16 compute mode;
  7. the loop the feature exists for: report -> observations.reject -> a second run on the same resident batch.

Every comparison prints its figure before it asserts; the figures of an MI355X run are in profiles/observation_weights.md.
"""
import numpy as np
import pytest

import gn_metric as M
import multiview_metric as X
import weights_ref as W
from conftest import golden, parity_log
from dsp_slam_amd import _lib as L, engine as E, observations as OBS, synth
from oracle import dsp_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
TRACE_KEYS = ("H", "b", "dx", "V", "K", "t_obj_cam", "code")


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _joint(eng, objs, prm, trace=True):
    return eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                     [np.zeros(64, F32) for _ in objs], trace=trace)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _run(b, n_it, keys=TRACE_KEYS):
    b.run()
    out = list(b.results())
    for e in range(n_it):
        tr = b.trace(e)
        out += [tr[k] for k in keys]
    return out


def _weights(rng, n, zeros=0.1):
    """Uniform in [0.1, 4], `zeros` of them exactly 0."""
    w = rng.uniform(0.1, 4.0, n).astype(F32)
    w[rng.random(n) < zeros] = 0.0
    return w


def _ragged_objects():
    return [synth.make_object(710, n_surface=120, n_background=40, n_foreground=60), synth.make_object(711, n_surface=97, n_background=35, n_foreground=70),
            synth.make_object(712, n_surface=150, n_background=30)]


# ---- 1. unit weights -------------------------------------------------------------------------------------------------------------------
def test_unit_weights_joint_is_the_plain_run(eng):
    objs = _ragged_objects()
    n_it = 3
    prm = E.gn_params(num_iterations=n_it)
    b = _joint(eng, objs, prm)
    plain = _run(b, n_it)
    launches = [b.stats()[k] for k in ("n_mlp_fwd_launches", "n_mlp_jac_launches", "n_mlp_prepass_launches")]
    assert plain[3].tolist() == [0, 0, 0]
    for pw, rw in (([np.ones(o["pts"].shape[0], F32) for o in objs], [np.ones(o["rays"].shape[0], F32) for o in objs]),
                   (np.ones(sum(o["pts"].shape[0] for o in objs), F32), None), (None, np.ones(sum(o["rays"].shape[0] for o in objs), F32))):
        b.set_observation_weights(pw, rw)
        assert _same(plain, _run(b, n_it))
    b.set_observation_weights(None, None)                   # cleared again
    assert _same(plain, _run(b, n_it))
    assert launches == [b.stats()[k] for k in ("n_mlp_fwd_launches", "n_mlp_jac_launches", "n_mlp_prepass_launches")]
    b.close()


def test_unit_weights_pose_only_with_the_inlier_filter_is_the_plain_run(eng):
    g = golden("golden_pose_only_8it.npz")
    prm = E.gn_params(pose_only_iterations=8)
    b = eng.pose_batch(prm, [g["t_co_se3"]], [float(g["scale"])], [g["pts"]], [g["code"]], trace=True)
    plain = _run(b, 8)
    assert int(b.trace(7)["K"][0]) < g["pts"].shape[0]          # the filter dropped points
    b.set_observation_weights(np.ones(g["pts"].shape[0], F32), np.ones(7, F32))      # a pose-only batch ignores ray_w
    assert _same(plain, _run(b, 8))
    b.set_observation_weights()
    assert _same(plain, _run(b, 8))
    b.close()


def test_unit_weights_three_views_is_the_plain_run(eng):
    case = X.case_three_views()
    obj = case["objects"][0]
    prm = E.gn_params(num_iterations=case["n_it"], **X.HYPER)
    b = eng.multiview_batch(prm, [obj["t"]], [obj["views"]], trace=True)

    def run():
        b.run()
        out = list(b.results())
        for e in range(case["n_it"]):
            tr, tv = b.trace(e), b.trace_views(e)
            out += [tr[k] for k in TRACE_KEYS] + [tv[k] for k in sorted(tv)]
        return out
    plain = run()
    b.set_observation_weights([np.ones(v["pts"].shape[0], F32) for v in obj["views"]], [np.ones(v["rays"].shape[0], F32) for v in obj["views"]])
    assert _same(plain, run())
    b.set_observation_weights(None, None)
    assert _same(plain, run())
    b.close()


# ---- 2. zero rays equal removal, bit for bit -------------------------------------------------------------------------------------------
def _without_rays(o, keep):
    n_fg = o["depth"].shape[0]
    return dict(o, rays=o["rays"][keep], depth=o["depth"][keep[:n_fg]])


def _zero_rays_equal_removal(eng, n_depth, which, configure=None):
    """configure(b, objs): called on each of the two batches before it runs (tests/test_gpu_feature_forms.py pins a launch form there); what
    it returns, if callable, is called on the batch after the run."""
    if which == "one_latency_sized":
        objs = [synth.make_object(720, n_surface=250, n_background=150, n_foreground=300)]
        assert objs[0]["rays"].shape[0] == 450
    else:
        objs = _ragged_objects()
    rng = np.random.default_rng(3)
    keep = [rng.random(o["rays"].shape[0]) >= 1 / 3 for o in objs]          # about a third of the rays, foreground and background alike
    for o, k in zip(objs, keep):
        n_fg = o["depth"].shape[0]
        assert (~k[:n_fg]).sum() > 0 and (~k[n_fg:]).sum() > 0
    n_it = 3
    prm = E.gn_params(num_iterations=n_it, num_depth_samples=n_depth)
    keys = ("H", "b", "dx", "V", "K", "m", "t_obj_cam", "code", "depths")       # (not set_sums: the checksums hash the ray's index)
    out = []
    for weighted in (True, False):
        objs_ = objs if weighted else [_without_rays(o, k) for o, k in zip(objs, keep)]
        b = _joint(eng, objs_, prm)
        after = configure(b, objs_) if configure is not None else None
        if weighted:
            b.set_observation_weights(None, [k.astype(F32) for k in keep])
        out.append(_run(b, n_it, keys))
        if callable(after):
            after(b)
        b.close()
    weighted, reduced = out
    print("zero rays, D=%d, %s: status %s, V %s K %s at the last iteration" % (n_depth, which, weighted[3], weighted[-6], weighted[-5]))
    assert weighted[3].tolist() == [0] * len(objs) and all((weighted[4 + len(keys) * e + 4] > 0).all() for e in range(n_it))
    assert _same(weighted, reduced)


@pytest.mark.parametrize("n_depth", [50, 64])
@pytest.mark.parametrize("which", ["one_latency_sized", "three_objects"])
def test_zero_rays_equal_removal_bit_for_bit(eng, n_depth, which):
    _zero_rays_equal_removal(eng, n_depth, which)


# ---- 3. weighted systems against fp64 --------------------------------------------------------------------------------------------------
WORST = {}


def _note(kind, rec):
    WORST[kind] = max(WORST.get(kind, 0.0), max(v for k, v in rec.items() if k.startswith("dev_") and k != "dev_solve"))
    print("worst scaled error so far (%s): %.3e" % (kind, WORST[kind]))


def _metric_objects():
    """(points, rays): 40 points leave Gram slices empty, 513 give a second row group, 2100 a second 128-row stage; 30 and 450 rays."""
    return [synth.make_object(731, n_surface=40, n_background=8, n_foreground=22), synth.make_object(732, n_surface=513, n_background=150, n_foreground=300),
            synth.make_object(733, n_surface=2100, n_background=150, n_foreground=300)]


def _check_joint_state(eng, dec, objs, prm, oprm, pw, rw, t, code, depths, want=None, label="", kind="joint", configure=None, check=None):
    """One iteration of a batch of `objs` with the weights (pw, rw per object; None = no weights) from the injected state, every object's
    system against the weighted fp64 reference on the device's own sets.  want: the (H, b, dx) bits the iteration must reproduce.
    configure(b): called on the batch before it runs (tests/test_gpu_feature_forms.py pins a launch form there); what it returns, if
    callable, is called on the batch after the run (the stats of the form that ran); check: the objects held to fp64 (None = all).  -> the iteration's trace."""
    n_d = oprm.num_depth_samples
    b = _joint(eng, objs, prm)
    after = configure(b) if configure is not None else None
    if pw is not None or rw is not None:
        b.set_observation_weights(pw, rw)
    b.set_start_state(t, code, depths)
    b.set_iterations(1)
    b.run()
    tr = b.trace(0)
    if callable(after):
        after(b)
    if want is not None:
        assert all(np.array_equal(tr[k], want[k]) for k in ("H", "b", "dx", "V", "K")), "the re-run from the traced state does not reproduce the traced system"
    for i, o in enumerate(objs):
        if check is not None and i not in check:
            continue
        m, _, deds = b.debug_samples(i, o["rays"].shape[0], n_d)
        sets = W.device_sets(m, deds)
        assert sets["valid"][0].shape[0] == int(tr["V"][i]) and sets["kept"][0].shape[0] == int(tr["K"][i])
        if rw is not None and rw[i] is not None:
            assert not m[np.asarray(rw[i]) == 0].any(), "a ray of weight 0 was sampled"
        lin = W.linearise(dec, oprm, o["pts"], o["rays"], o["depth"], t[i], code[i], depths[i][:n_d], sets, None if pw is None else pw[i], None if rw is None else rw[i])
        dev = dict(H=tr["H"][i], b=tr["b"][i], dx=tr["dx"][i])
        print("%s object %d (%d points, %d rays): V %d K %d Mw %.6g Kw %.6g: %s" % (label, i, o["pts"].shape[0], o["rays"].shape[0], tr["V"][i], tr["K"][i], lin["Mw"],
                                                                                  lin["Kw"], M.flat(M.scaled_errors(dev, lin, oprm.k4))))
        rec = M.check_against_fp64(dev, lin, oprm.k4, what="%s object %d" % (label, i))
        _note(kind, rec)
        parity_log(kind="weights_fp64", case=label, object=i, **rec)
    b.close()
    return tr


def test_weighted_joint_systems_against_fp64(eng, oracle_decoder):
    objs = _metric_objects()
    assert [(o["pts"].shape[0], o["rays"].shape[0]) for o in objs] == [(40, 30), (513, 450), (2100, 450)]
    rng = np.random.default_rng(11)
    pw = [_weights(rng, o["pts"].shape[0]) for o in objs]
    rw = [_weights(rng, o["rays"].shape[0]) for o in objs]
    assert all((w == 0).any() for w in pw[1:] + rw[1:])
    n_it = 2
    prm, oprm = E.gn_params(num_iterations=n_it), O.GNParams(num_iterations=1)
    b = _joint(eng, objs, prm)
    b.set_observation_weights(pw, rw)
    b.run()
    assert b.results()[3].tolist() == [0, 0, 0]
    traces = [b.trace(e) for e in range(n_it)]
    b.close()
    for e, tr in enumerate(traces):
        _check_joint_state(eng, oracle_decoder, objs, prm, oprm, pw, rw, tr["t_obj_cam"], tr["code"], tr["depths"], want=tr, label="weighted joint iteration %d" % e)


def test_weighted_pose_only_systems_against_fp64(eng, oracle_decoder):
    g = golden("golden_pose_only_8it.npz")
    pts = g["pts"]
    pw = _weights(np.random.default_rng(12), pts.shape[0])
    prm = E.gn_params(pose_only_iterations=8)
    b = eng.pose_batch(prm, [g["t_co_se3"]], [float(g["scale"])], [pts], [g["code"]], trace=True)
    b.set_observation_weights(pw)
    b.set_report(True)
    b.run()
    alive = b.report()["pt_alive"]
    traces = [b.trace(e) for e in range(8)]
    b.close()
    print("weighted pose-only: %d of %d points alive behind the filter, %d of weight 0" % (alive.sum(), pts.shape[0], (pw == 0).sum()))
    assert 0 < alive.sum() < pts.shape[0]
    for e, tr in enumerate(traces):
        al = None if e <= 4 else alive                        # the filter runs behind iteration 4
        lin = W.pose_only(oracle_decoder, pts, tr["t_obj_cam"][0], g["code"], pw, al)
        assert int(tr["K"][0]) == (pts.shape[0] if al is None else int(alive.sum()))          # the count stays a count
        dev = W.embed6(tr["H"][0], tr["b"][0], tr["dx"][0])
        print("weighted pose-only iteration %d: Mw %.6g: %s" % (e, lin["Mw"], M.flat(M.scaled_errors(dev, lin, 0.0))))
        _note("pose_only", M.check_against_fp64(dev, lin, 0.0, what="weighted pose-only iteration %d" % e))


def _check_multiview_states(b, dec, oprm, objs, pw, rw, traces, n_d, check=None, zero_views=(), label="weighted multi-view", kind="multiview"):
    """Every traced iteration (trace, trace_views) of the weighted multi-view batch b run again from its traced state: the same bits, and the
    pooled system of every object (check: of these objects) against the weighted fp64 reference on the device's own per-view sets."""
    views = [v for o in objs for v in o["views"]]
    off = np.concatenate([[0], np.cumsum([len(o["views"]) for o in objs])]).astype(int)
    for e, (tr, tv) in enumerate(traces):
        assert all(int(tv["V"][k]) == 0 and int(tv["K"][k]) == 0 for k in zero_views)
        b.set_start_state(tr["t_obj_cam"], tr["code"], tv["depths"])
        b.set_iterations(1)
        b.run()
        tr1, tv1 = b.trace(0), b.trace_views(0)
        assert all(np.array_equal(tr1[k], tr[k]) for k in ("H", "b", "dx", "V", "K")) and np.array_equal(tv1["set_sums"], tv["set_sums"])
        for i, o in enumerate(objs):
            if check is not None and i not in check:
                continue
            rows = range(off[i], off[i + 1])
            sets = []
            for k in rows:
                m, _, deds = b.debug_samples(k, views[k]["rays"].shape[0], n_d)
                sets.append(W.device_sets(m, deds))
            lin = W.linearise_multiview(dec, oprm, o["views"], tr["t_obj_cam"][i], tr["code"][i], [tv["depths"][k][:n_d] for k in rows], sets,
                                        [pw[k] for k in rows], [rw[k] for k in rows])
            assert lin["K_views"] == [int(tv["K"][k]) for k in rows] and int(tr["K"][i]) == sum(lin["K_views"])
            dev = dict(H=tr["H"][i], b=tr["b"][i], dx=tr["dx"][i])
            print("%s iteration %d object %d (%d views): K %s Mw %.6g Kw %.6g: %s" % (label, e, i, len(o["views"]), lin["K_views"], lin["Mw"], lin["Kw"],
                                                                                      M.flat(M.scaled_errors(dev, lin, oprm.k4))))
            _note(kind, M.check_against_fp64(dev, lin, oprm.k4, what="%s iteration %d object %d" % (label, e, i)))


def test_weighted_ragged_multiview_systems_against_fp64(eng, oracle_decoder):
    case = X.case_ragged()
    objs = case["objects"]
    rng = np.random.default_rng(13)
    views = [v for o in objs for v in o["views"]]
    pw = [_weights(rng, v["pts"].shape[0]) for v in views]
    rw = [_weights(rng, v["rays"].shape[0]) for v in views]
    zero_view = 4                                            # the second of the last object's three views: all its weights 0
    pw[zero_view][:] = 0
    rw[zero_view][:] = 0
    prm, oprm = E.gn_params(num_iterations=case["n_it"], **X.HYPER), X.oracle_params(case)
    b = eng.multiview_batch(prm, [o["t"] for o in objs], [o["views"] for o in objs], trace=True)
    b.set_observation_weights(pw, rw)
    b.run()
    assert b.results()[3].tolist() == [0, 0, 0]
    traces = [(b.trace(e), b.trace_views(e)) for e in range(case["n_it"])]
    _check_multiview_states(b, oracle_decoder, oprm, objs, pw, rw, traces, case["n_depth"], zero_views=(zero_view,))
    b.close()


# ---- 4. zero points equal removal, within the metric -----------------------------------------------------------------------------------
def test_zero_points_equal_removal_within_the_metric(eng, oracle_decoder):
    o = synth.make_object(741, n_surface=513, n_background=100, n_foreground=200)
    keep = np.random.default_rng(4).random(513) >= 0.3
    red = dict(o, pts=o["pts"][keep])
    prm, oprm = E.gn_params(num_iterations=1), O.GNParams(num_iterations=1)
    b = _joint(eng, [o], prm)
    b.run()
    tr0 = b.trace(0)
    b.close()
    state = (tr0["t_obj_cam"], tr0["code"], tr0["depths"])
    a = _check_joint_state(eng, oracle_decoder, [o], prm, oprm, [keep.astype(F32)], None, *state, label="zero points, weighted", kind="zero_points")
    c = _check_joint_state(eng, oracle_decoder, [red], prm, oprm, None, None, *state, label="zero points, reduced batch", kind="zero_points")
    assert int(a["V"][0]) == int(c["V"][0]) and int(a["K"][0]) == int(c["K"][0]) and np.array_equal(a["set_sums"], c["set_sums"])
    # ... against the SAME fp64 system: the weighted reference on the full inputs is the plain reference on the reduced ones
    b = _joint(eng, [o], prm)
    b.set_start_state(*state)
    b.run()
    sets = W.device_sets(*[b.debug_samples(0, o["rays"].shape[0], 50)[k] for k in (0, 2)])
    b.close()
    lw = W.linearise(oracle_decoder, oprm, o["pts"], o["rays"], o["depth"], state[0][0], state[1][0], state[2][0][:50], sets, keep.astype(F32), None)
    lr = O.linearise_fp64(oracle_decoder, oprm, red["pts"], red["rays"], red["depth"], state[0][0], state[1][0], state[2][0][:50], sets)
    assert np.abs(lw["H"] - lr["H"]).max() <= 1e-11 * np.abs(lr["H"]).max() and np.abs(lw["b"] - lr["b"]).max() <= 1e-11 * np.abs(lr["b"]).max()


# ---- 5. degenerate sums and errors -----------------------------------------------------------------------------------------------------
def test_degenerate_sums(eng):
    objs = _ragged_objects()
    n_it = 2
    prm = E.gn_params(num_iterations=n_it)
    b = _joint(eng, objs, prm)
    plain = _run(b, n_it)
    ones_p = [np.ones(o["pts"].shape[0], F32) for o in objs]
    ones_r = [np.ones(o["rays"].shape[0], F32) for o in objs]
    b.set_observation_weights([np.zeros_like(ones_p[0])] + ones_p[1:], ones_r[:2] + [np.zeros_like(ones_r[2])])
    b.set_report(True)
    got = _run(b, n_it)
    rep = b.report()
    assert got[3].tolist() == [L.OBJ_NAN, 0, L.OBJ_FEW_SAMPLES]
    assert all(np.array_equal(p[1], q[1], equal_nan=True) for p, q in zip(plain, got))        # the neighbour keeps its bits
    assert rep["status"].tolist() == [L.OBJ_NAN, 0, L.OBJ_FEW_SAMPLES] and rep["V"][2] == 0
    # one zero ray of a good object: the rows of a member without a render term
    rw = [w.copy() for w in ones_r]
    rw[1][[0, 80]] = 0
    b.set_observation_weights(None, rw)
    b.run()
    rep = b.report()
    r0 = rep["ray_off"][1]
    for key in ("ray_depth", "ray_hit", "ray_residual"):
        assert np.isnan(rep[key][[r0, r0 + 80]]).all() and np.isfinite(np.delete(rep[key][r0:rep["ray_off"][2]], [0, 80])).all(), key
    assert not rep["ray_counts"][[r0, r0 + 80]].any() and rep["K"][1] == rep["ray_counts"][r0:rep["ray_off"][2], 2].sum()
    b.close()


def test_refused_weights_keep_the_previous_setting(eng):
    o = _ragged_objects()[0]
    n_it = 2
    prm = E.gn_params(num_iterations=n_it)
    b = _joint(eng, [o], prm)
    w = _weights(np.random.default_rng(5), o["pts"].shape[0])
    b.set_observation_weights(w, None)
    want = _run(b, n_it)
    for bad in (-1.0, np.nan, np.inf):
        x = np.ones(o["rays"].shape[0], F32)
        x[7] = bad
        with pytest.raises(L.DspError):
            b.set_observation_weights(None, x)
        y = np.ones(o["pts"].shape[0], F32)
        y[7] = bad
        with pytest.raises(L.DspError):
            b.set_observation_weights(y, None)
    with pytest.raises(ValueError):
        b.set_observation_weights(np.ones(3, F32), None)
    assert _same(want, _run(b, n_it))
    b.close()


def test_an_allocation_failure_leaves_weights_off_and_the_batch_running(eng):
    o = _ragged_objects()[0]
    n_it = 2
    prm = E.gn_params(num_iterations=n_it)
    b = _joint(eng, [o], prm)
    plain = _run(b, n_it)
    w = _weights(np.random.default_rng(6), o["pts"].shape[0])
    eng.trim()
    eng.fail_alloc(1)
    rc = L.load().dsp_batch_observation_weights(b._h, L.ptr(w), None)
    eng.fail_alloc(-1)
    assert rc == -3 and b"out of device memory" in L.load().dsp_last_error(eng._h)          # DSP_E_NOMEM
    assert _same(plain, _run(b, n_it))                       # weights off, the batch usable
    b.set_observation_weights(w, None)
    got = _run(b, n_it)
    assert got[3].tolist() == [0] and not np.array_equal(got[0], plain[0])
    b.close()


# ---- 6. with the other features --------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return float(np.spacing(np.abs(F32(x))))


def test_with_the_report_and_the_posterior(eng, oracle_decoder):
    objs = _ragged_objects()[:2]
    rng = np.random.default_rng(21)
    pw = [_weights(rng, o["pts"].shape[0]) for o in objs]
    rw = [_weights(rng, o["rays"].shape[0]) for o in objs]
    n_it = 3
    prm, oprm = E.gn_params(num_iterations=n_it), O.GNParams(num_iterations=1)
    recs = {}
    for weights in ("mean", "sum"):
        b = _joint(eng, objs, prm)
        b.set_observation_weights(pw, rw)
        b.set_posterior(2, weights)
        b.set_report(True)
        b.run()
        recs[weights] = rec = b.posterior()
        rep = b.report()
        assert rec["status"].tolist() == [0, 0]
        for i, o in enumerate(objs):
            kc = rep["ray_counts"][rep["ray_off"][i]:rep["ray_off"][i + 1], 2]
            assert rep["K"][i] == kc.sum() == rec["K"][i] and rep["M"][i] == o["pts"].shape[0] == rec["M"][i]          # the counts stay counts
            assert not kc[rw[i] == 0].any()
            # the loss identity with the weight sums, formed from the weights, the alive bits and ray_counts[:, 2]
            mw = float(np.sum(pw[i].astype(np.float64) * rep["pt_alive"][rep["pts_off"][i]:rep["pts_off"][i + 1]]))
            kw = float(np.sum(rw[i].astype(np.float64) * kc))
            loss = F32(prm.k1) * (F32(rep["sum_r"][i]) / F32(kw)) + F32(prm.k2) * (F32(rep["sum_s"][i]) / F32(mw))
            print("weighted loss identity (%s) object %d: from the sums %.9g, posterior %.9g, %.2f ulp32" % (
                weights, i, loss, rec["loss"][i], abs(float(loss) - float(rec["loss"][i])) / _ulp32(rec["loss"][i])))
            assert abs(float(loss) - float(rec["loss"][i])) <= 4 * _ulp32(rec["loss"][i])
            # Lambda against the weighted fp64 reference at the record's state, on the device's sets there
            m, _, deds = b.debug_samples(i, o["rays"].shape[0], 50)
            sets = W.device_sets(m, deds)
            assert sets["kept"][0].shape[0] == rec["K"][i]
            lin = W.linearise(oracle_decoder, oprm, o["pts"], o["rays"], o["depth"], rec["t_obj_cam"][i], rec["code"][i], rec["depths"][i][:50], sets, pw[i], rw[i])
            f_s, f_r = (lin["Mw"], lin["Kw"]) if weights == "sum" else (1.0, 1.0)            # SUM: k2 / k1 on the weighted Grams
            ref = f_s * lin["Ds"] + f_r * lin["Dr"] + lin["H_code_prior"] + lin["H_rot"]
            dsum = np.diag(f_s * lin["Ds"] + f_r * lin["Dr"])
            sh = np.sqrt(np.outer(dsum, dsum))
            allow = 4 * M.ulp32(ref) + M._rot_allowances(lin, oprm.k4)[0] + max(f_s, f_r) * lin["H_flip"]
            scaled = np.maximum(np.abs(rec["Lambda"][i] - ref) - allow, 0) / np.maximum(sh, 1e-300)
            print("weighted %s Lambda object %d against fp64: worst scaled error %.2e (TAU_H %.1e)" % (weights, i, scaled.max(), M.TAU_H))
            WORST["posterior_" + weights] = max(WORST.get("posterior_" + weights, 0.0), float(scaled.max()))
            assert scaled.max() <= M.TAU_H
        b.close()
    assert _same([recs["mean"][k] for k in ("t_obj_cam", "code", "loss")], [recs["sum"][k] for k in ("t_obj_cam", "code", "loss")])


def test_with_step_control_the_costs_are_the_weighted_losses(eng):
    o = _ragged_objects()[0]
    rng = np.random.default_rng(22)
    pw, rw = _weights(rng, o["pts"].shape[0]), _weights(rng, o["rays"].shape[0])
    n_it = 4
    prm = E.gn_params(num_iterations=n_it)
    b = _joint(eng, [o], prm)
    b.set_observation_weights(pw, rw)
    b.set_step_control(0.0, 10.0, 0.1, 1.0, float("inf"))
    b.run()
    log = b.step_log()
    traces = [b.trace(e) for e in range(n_it)]
    assert b.results()[3].tolist() == [0] and (log["decision"] != 0).all()
    # the cost of iteration e is the weighted loss AT the state iteration e linearised: a plain weighted one-iteration run from it returns it
    for e in range(n_it):
        c = _joint(eng, [o], E.gn_params(num_iterations=1))
        c.set_observation_weights(pw, rw)
        c.set_start_state(traces[e]["t_obj_cam"], traces[e]["code"], traces[e]["depths"])
        c.run()
        loss = c.results()[2][0]
        c.close()
        print("step control iteration %d: cost %.9g, the weighted loss at that state %.9g" % (e, log["cost"][e, 0], loss))
        assert F32(log["cost"][e, 0]) == loss
    b.set_observation_weights()
    b.run()
    assert not np.array_equal(b.step_log()["cost"], log["cost"])
    b.close()


@pytest.mark.parametrize("prior", [False, True])
def test_with_the_convergence_rule_and_the_prior(eng, prior):
    """A weighted run under the convergence rule (tolerances taken from the steps of its own unstopped run, as tests/test_gpu_early_stop.py
    takes them) freezes early and returns its own shorter run bit for bit -- with a prior too."""
    o = _ragged_objects()[0]
    rng = np.random.default_rng(23)
    pw, rw = _weights(rng, o["pts"].shape[0]), _weights(rng, o["rays"].shape[0])
    n_it = 8
    prm = E.gn_params(num_iterations=n_it)
    b = _joint(eng, [o], prm)
    b.set_observation_weights(pw, rw)
    if prior:
        b.set_posterior(2, "mean")
        b.run()
        rec = b.posterior()
        assert rec["status"].tolist() == [0]
        b.set_posterior(0, "mean")
        b.set_prior(rec["t_obj_cam"], rec["code"], rec["Lambda"])
    b.run()
    unstopped = b.results()
    assert unstopped[3].tolist() == [0] and int(b.iterations_used()[0]) == n_it
    dx = np.abs(b.trace(n_it - 3)["dx"][0])
    tp, tc = 1.01 * float(dx[:7].max()), 1.01 * float(dx[7:].max())
    b.set_convergence(tp, tc, 1)
    b.run()
    stopped, used = b.results(), int(b.iterations_used()[0])
    print("weighted, convergence rule%s: tolerances %.3g / %.3g, %d of %d iterations used" % (", prior" if prior else "", tp, tc, used, n_it))
    assert stopped[3].tolist() == [0] and 1 <= used <= n_it - 2
    b.set_convergence(0.0, 0.0, 1)
    b.set_iterations(used)
    b.run()
    assert _same(stopped, b.results()) and not _same(stopped, unstopped)
    b.close()


def test_a_partial_rerun_after_a_guard_trip_keeps_the_weights(oracle_decoder):
    """A forced bf16 margin of 2e-5 trips the prepass guard (tests/test_gpu_report.py): the tripped objects run again with the prepass off.
    With weights set, every object's result row is the weighted prepass-off run's, bit for bit."""
    objs = _ragged_objects()
    rng = np.random.default_rng(24)
    pw = [_weights(rng, o["pts"].shape[0]) for o in objs]
    rw = [_weights(rng, o["rays"].shape[0]) for o in objs]
    prm = E.gn_params(num_iterations=3)
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    out = {}
    for name, mode, delta, weighted in (("off", L.PREPASS_OFF, -1.0, True), ("trip", L.PREPASS_BF16, 2e-5, True), ("plain", L.PREPASS_OFF, -1.0, False)):
        b = _joint(own, objs, prm, trace=False)
        b.set_prepass(mode, delta)
        if weighted:
            b.set_observation_weights(pw, rw)
        b.run()
        out[name] = (b.results(), b.stats())
        b.close()
    own.close()
    st = out["trip"][1]
    print("weighted, guard trips", st["prepass_guard_trips"], "objects re-run", st["prepass_guard_objects"], "of", len(objs))
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_trips"] > 0 and st["prepass_guard_objects"] > 0
    assert out["off"][0][3].tolist() == [0, 0, 0]
    assert _same(out["trip"][0], out["off"][0]) and not _same(out["off"][0], out["plain"][0])


def test_in_the_low_precision_compute_mode(eng):
    """The f16 compute mode takes weights like the fp32 path (no accuracy is claimed for its values): unit weights are its plain run bit
    for bit, drawn weights change the result, zero rays equal removal."""
    objs = _ragged_objects()
    prm = E.gn_params(num_iterations=3)
    rng = np.random.default_rng(25)
    keep = [rng.random(o["rays"].shape[0]) >= 1 / 3 for o in objs]

    def run(objs_, pw=None, rw=None):
        b = _joint(eng, objs_, prm, trace=False)
        b.set_compute(L.COMPUTE_F16)
        b.set_lp_small_batches(1)
        if pw is not None or rw is not None:
            b.set_observation_weights(pw, rw)
        b.run()
        res = b.results()
        b.close()
        return res
    plain = run(objs)
    assert plain[3].tolist() == [0, 0, 0]
    assert _same(plain, run(objs, [np.ones(o["pts"].shape[0], F32) for o in objs], [np.ones(o["rays"].shape[0], F32) for o in objs]))
    drawn = run(objs, [_weights(rng, o["pts"].shape[0]) for o in objs], None)
    assert drawn[3].tolist() == [0, 0, 0] and not _same(plain, drawn)
    assert _same(run(objs, None, [k.astype(F32) for k in keep]), run([_without_rays(o, k) for o, k in zip(objs, keep)]))


# ---- 7. the loop it exists for ---------------------------------------------------------------------------------------------------------
LOOP_SEED = 756          # chosen on the CPU oracle (profiles/observation_weights.md: five of the eight seeds 751..758 improve in all three measures)
PT_SDF_MAX, RAY_RES_MAX = 0.025, 0.30      # the Huber threshold b2 of the surface term; the clip of the depth residual (loss.py:139-140)


def loop_case(seed):
    """A clean object and its corrupted twin: 25 % of the surface points displaced by 0.3 object units (along the viewing ray), 25 % of the
    foreground depths offset by 0.5."""
    clean = synth.make_object(seed, n_surface=400, n_background=120)
    rng = np.random.default_rng(seed)
    scale = float(np.cbrt(np.linalg.det(clean["t_cam_obj_gt"][:3, :3])))
    pts, depth = clean["pts"].copy(), clean["depth"].copy()
    bad_p = rng.permutation(pts.shape[0])[:pts.shape[0] // 4]
    pts[bad_p] += (F32(0.3 * scale) * pts[bad_p] / np.linalg.norm(pts[bad_p], axis=1, keepdims=True)).astype(F32)
    bad_d = rng.permutation(depth.shape[0])[:depth.shape[0] // 4]
    depth[bad_d] += F32(0.5)
    return clean, dict(clean, pts=pts, depth=depth), bad_p, bad_d


def distances(res, ref):
    """(translation, rotation angle, code distance) between two results()."""
    ta, tb = res[0][0].astype(np.float64), ref[0][0].astype(np.float64)
    ra, rb = ta[:3, :3] / np.cbrt(np.linalg.det(ta[:3, :3])), tb[:3, :3] / np.cbrt(np.linalg.det(tb[:3, :3]))
    ang = float(np.arccos(np.clip((np.trace(ra @ rb.T) - 1) / 2, -1, 1)))
    return float(np.linalg.norm(ta[:3, 3] - tb[:3, 3])), ang, float(np.linalg.norm(res[1][0].astype(np.float64) - ref[1][0]))


def run_loop(eng, seed, n_it=10):
    clean, dirty, bad_p, bad_d = loop_case(seed)
    prm = E.gn_params(num_iterations=n_it)
    b = _joint(eng, [clean], prm, trace=False)
    b.run()
    ref = b.results()
    b.close()
    b = _joint(eng, [dirty], prm, trace=False)
    b.set_report(True)
    b.run()
    first = b.results()
    pt_w, ray_w = OBS.reject(b.report(), PT_SDF_MAX, RAY_RES_MAX)
    b.set_observation_weights(pt_w, ray_w)              # nothing re-uploaded but the two weight arrays
    b.run()
    second = b.results()
    b.close()
    hit_p = float((pt_w[bad_p] == 0).mean()), float((np.delete(pt_w, bad_p) == 0).mean())
    hit_d = float((ray_w[bad_d] == 0).mean()), float((np.delete(ray_w, bad_d) == 0).mean())
    return ref, first, second, hit_p, hit_d


def test_report_then_reject_then_rerun_moves_towards_the_clean_result(eng):
    ref, first, second, hit_p, hit_d = run_loop(eng, LOOP_SEED)
    assert ref[3].tolist() == [0] and first[3].tolist() == [0] and second[3].tolist() == [0]
    d1, d2 = distances(first, ref), distances(second, ref)
    print("the loop, seed %d: rejected %.0f %% of the displaced points (%.1f %% of the others), %.0f %% of the offset depths (%.1f %% of the others)" % (
        LOOP_SEED, 100 * hit_p[0], 100 * hit_p[1], 100 * hit_d[0], 100 * hit_d[1]))
    for name, a, c in zip(("translation", "rotation angle", "code distance"), d1, d2):
        print("the loop: %s to the clean-data result: unweighted %.6g, after reject %.6g" % (name, a, c))
    assert all(c < a for a, c in zip(d1, d2))


def test_worst_scaled_errors_are_printed():
    """(runs last in this file) The worst scaled errors tests 3, 4 and 6 measured, for profiles/observation_weights.md."""
    print("worst scaled errors against the weighted fp64 reference: %s" % {k: "%.3e" % v for k, v in sorted(WORST.items())})
    parity_log(kind="weights_worst", **WORST)
