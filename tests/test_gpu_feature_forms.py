"""GPU: observation weights, the report, the posterior pass, the prior, step control and the mask of unknowns in EVERY launch form.

The features' own tests run batches of one to three small objects with nothing pinned, whose plan (csrc/launch_plan.h) is always wave
bookkeeping, latency or cluster tiles, the speculative band and one whole prepass launch; the block form's kernels (k_sample_count,
k_render_write, the scan launches), the throughput form of mask reuse, fixed and hint passes never ran with a feature on.  Here every named
form of tests/launch_forms.py is pinned on resident batches with the features on and held, bit for bit, to the automatic plan's run;
tests/test_feature_forms_plan.py shows on the CPU that each form's pins reach its plan on these very shapes, and every run asserts from
stats() that the form ran (decoder launches per kind as the plan implies them, render rows counted on their own exactly with mask reuse,
cluster tiles, the prepass mode, no guard trip).

  a. weights, every form: results, traces (H, b, dx, V, K, t_obj_cam, code, depths, set_sums), iterations used; no sample on a zero ray;
  b. weights against the weighted fp64 reference (tests/weights_ref.py through gn_metric.check_against_fp64, TAU_H / TAU_B / TAU_SOLVE as
     they stand, pair=None) in the throughput and block + tail-split forms, and on 17 objects whose automatic plan is block bookkeeping +
     throughput mask reuse -- each of the 17 also bit-equal to its run alone (wave bookkeeping, cluster tiles, speculative band);
  c. zero-weight rays equal removal in the block and throughput forms, 50 and 64 depth samples;
  d. report + level-2 posterior record, every form, weights on and off; the throughput form against the host arithmetic;
  e. step control with rejected trials under hint passes (prepass on and off), ten fixed passes, block and throughput;
  f. everything on at once; g. an 18-view multi-view batch (automatic: block bookkeeping); h. pose-only across the inlier filter;
  i. the f16 compute mode, wave against block bookkeeping.

Left out of the bit comparisons, as documented: `m` (include/dsp_gn.h) and the report's band count ("Observation report": samples
behind a ray's first solid sample are not decoded under early ray termination or the prepass) -- the band count is compared between forms
whose plans decode the same samples (same prepass mode, same passes).  Every comparison prints its figure or the first differing key
before it asserts; the figures of an MI355X run are in profiles/feature_forms.md.
"""
import numpy as np
import pytest

import gn_metric as M
import launch_forms as F
import multiview_metric as X
import test_gpu_early_stop as ES
import test_gpu_multiview as TM
import test_gpu_prior as TP
import test_gpu_report as TR
import test_gpu_step_control as SC
import test_gpu_weights as TW
from conftest import golden, parity_log
from dsp_slam_amd import _lib as L, engine as E
from oracle import dsp_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
TRACE_KEYS = ("H", "b", "dx", "V", "K", "t_obj_cam", "code", "depths", "set_sums")
VIEW_KEYS = ("V", "K", "t_obj_cam", "set_sums", "depths")
REPORT_KEYS = tuple(k for k in TR.REPORT_KEYS if k not in ("ray_counts", "m"))
BAND = "report.band_count"
EVIDENCE = []


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


# ---- what a run returns, by name -------------------------------------------------------------------------------------------------------------
def collect(b, n_it, views=False, report=False, posterior=False, prior=False, steps=False, trace=True):
    out = dict(zip(("t_cam_obj", "code", "loss", "status"), b.results()))
    out["iterations_used"] = b.iterations_used()
    for e in range(n_it if trace else 0):
        tr = b.trace(e)
        out.update({"trace[%d].%s" % (e, k): tr[k] for k in TRACE_KEYS})
        if views:
            tv = b.trace_views(e)
            out.update({"trace_views[%d].%s" % (e, k): tv[k] for k in VIEW_KEYS})
    if report:
        rep = b.report()
        out.update({"report.%s" % k: rep[k] for k in REPORT_KEYS})
        out["report.in_sphere_count"], out[BAND], out["report.kept_count"] = (np.ascontiguousarray(rep["ray_counts"][:, j]) for j in range(3))
    if posterior:
        rec = b.posterior()
        out.update({"posterior.%s" % k: rec[k] for k in TR.POST_KEYS})
    if prior:
        pr = b.prior_residual()
        out.update({"prior.e": pr["e"], "prior.chi2": pr["chi2"]})
    if steps:
        sl = b.step_log()
        out.update({"step_log.%s" % k: sl[k] for k in ("decision", "cost", "lambda")})
    return out


def same_samples(p, q):
    """Two plans decode the same ray samples: the same prepass kernel and the same passes."""
    return all(p[k] == q[k] for k in ("prepass_mode", "fixed_passes", "hint_passes", "whole", "lp_compute"))


def assert_same_bits(what, got, ref, band=False):
    assert list(got) == list(ref), (what, set(got) ^ set(ref))
    keys = [k for k in ref if band or k != BAND]
    diff = [k for k in keys if not TR._bits(got[k], ref[k])]
    if BAND in ref and not band:
        print("%s: band counts (informational) %s" % (what, "equal" if np.array_equal(got[BAND], ref[BAND]) else "differ on %d rays" % (got[BAND] != ref[BAND]).sum()))
    if diff:
        k = diff[0]
        a, c = np.asarray(got[k], np.float64).ravel(), np.asarray(ref[k], np.float64).ravel()
        bad = np.flatnonzero(~((a == c) | (np.isnan(a) & np.isnan(c))))
        print("%s: %d of %d keys differ; first %s: %d of %d entries, first at %d: %r != %r" % (what, len(diff), len(keys), k, bad.size, a.size, bad[0] if bad.size else -1,
                                                                                                a[bad[0]] if bad.size else None, c[bad[0]] if bad.size else None))
    else:
        print("%s: %d arrays bit-equal" % (what, len(keys)))
    assert not diff, (what, diff[:6])


def evidence(name, shape_name, shape, form, plan, b, fronts, rows_expected=True, must_cluster=False, **kw):
    st = b.stats()
    ev = F.check_stats(form or "automatic", plan, st, fronts, rows_expected, must_cluster=must_cluster and form == "cluster_on")
    ev.update(test=name, shape=shape_name, plan={k: v for k, v in plan.items() if v and k != "cluster_max_tiles"}, **kw)
    EVIDENCE.append(ev)
    parity_log(kind="feature_forms", **ev)
    return st


def every_form(name, b, shape_name, shape, run, fronts, forms=None, must_cluster=False, before=None):
    """The automatic plan's run of b, then every form pinned in turn (and put back): run(b) -> dict of arrays, all bit-equal to the
    automatic run's.  before(form): called behind each run with the batch still as that run left it.  -> the automatic run's arrays."""
    auto_plan = F.plan_of(shape)
    ref = run(b)
    evidence(name, shape_name, shape, None, auto_plan, b, fronts)
    if before:
        before(None, auto_plan)
    for form in (F.uses(shape_name, shape) if forms is None else forms):
        pins = F.FORMS[form]["pins"]
        plan = F.plan_of_form(shape, form)
        assert all(plan[k] == v for k, v in F.FORMS[form]["plan"].items()), (form, plan)
        F.pin(b, pins)
        got = run(b)
        evidence(name, shape_name, shape, form, plan, b, fronts, must_cluster=must_cluster)
        if before:
            before(form, plan)
        F.unpin(b, pins)
        assert_same_bits("%s %s %s" % (name, shape_name, form), got, ref, band=same_samples(plan, auto_plan))
    got = run(b)          # every pin is back at automatic: the first run again
    assert_same_bits("%s %s automatic again" % (name, shape_name), got, ref, band=True)
    return ref


def _objects(shape_name):
    return dict(ragged3=F.ragged3, detection=F.detection, hinted3=F.hinted3)[shape_name]()


def _drawn_weights(objs, seed):
    rng = np.random.default_rng(seed)
    pw = [TW._weights(rng, o["pts"].shape[0]) for o in objs]
    rw = [TW._weights(rng, o["rays"].shape[0]) for o in objs]
    assert (np.concatenate(pw) == 0).sum() >= 3 and (np.concatenate(rw) == 0).sum() >= 3 and (rw[0] == 0).any()
    return pw, rw


# ---- a. weights, every form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_name", ["ragged3", "detection", "hinted3"])
def test_a_weights_in_every_form(eng, shape_name):
    objs = _objects(shape_name)
    shape = F.shape_of(F.sizes(objs))
    pw, rw = _drawn_weights(objs, 31)
    n_it = 3
    b = TW._joint(eng, objs, E.gn_params(num_iterations=n_it))
    b.set_observation_weights(pw, rw)

    def no_sample_on_a_zero_ray(form, plan):
        for i, o in enumerate(objs):
            m = b.debug_samples(i, o["rays"].shape[0], 50)[0]
            assert m.any() and not m[rw[i] == 0].any(), "%s: a ray of weight 0 was sampled (object %d)" % (form, i)
    ref = every_form("a", b, shape_name, shape, lambda b: (b.run(), collect(b, n_it))[1], n_it, must_cluster=shape_name != "hinted3", before=no_sample_on_a_zero_ray)
    b.close()
    assert ref["status"].tolist() == [0] * len(objs) and (ref["iterations_used"] == n_it).all()
    assert all((ref["trace[%d].K" % e] > 0).all() for e in range(n_it))


# ---- b. weights against fp64 in the throughput and block forms -----------------------------------------------------------------------------------
def _pinned(name, shape_name, shape, form, fronts):
    """configure(b) for tests/test_gpu_weights._check_joint_state: pin `form` (None: nothing) in front of the run, show behind it that it ran."""
    def configure(b):
        plan = F.plan_of_form(shape, form)
        if form:
            assert all(plan[k] == v for k, v in F.FORMS[form]["plan"].items()), (form, plan)
            F.pin(b, F.FORMS[form]["pins"])
        return lambda b: evidence(name, shape_name, shape, form, plan, b, fronts)
    return configure


@pytest.mark.parametrize("form", ["throughput", "block+tail_split"])
def test_b_weighted_systems_against_fp64_in_the_form(eng, oracle_decoder, form):
    objs = F.metric3()
    shape = F.shape_of(F.sizes(objs))
    rng = np.random.default_rng(11)
    pw = [TW._weights(rng, o["pts"].shape[0]) for o in objs]
    rw = [TW._weights(rng, o["rays"].shape[0]) for o in objs]
    n_it = 2
    prm, oprm = E.gn_params(num_iterations=n_it), O.GNParams(num_iterations=1)
    b = TW._joint(eng, objs, prm)
    after = _pinned("b", "metric3", shape, form, n_it)(b)
    b.set_observation_weights(pw, rw)
    b.run()
    after(b)
    assert b.results()[3].tolist() == [0, 0, 0]
    traces = [b.trace(e) for e in range(n_it)]
    b.close()
    for e, tr in enumerate(traces):
        TW._check_joint_state(eng, oracle_decoder, objs, prm, oprm, pw, rw, tr["t_obj_cam"], tr["code"], tr["depths"], want=tr,
                              label="weighted joint, %s, iteration %d" % (form, e), kind="forms/joint/" + form, configure=_pinned("b", "metric3", shape, form, 1))


def test_b_seventeen_objects_in_the_automatic_block_and_throughput_plan(eng, oracle_decoder):
    objs = F.auto_block17()
    shape = F.shape_of(F.sizes(objs))
    pw, rw = _drawn_weights(objs, 32)
    n_it = 2
    prm, oprm = E.gn_params(num_iterations=n_it), O.GNParams(num_iterations=1)
    plan = F.plan_of(shape)
    assert plan["bookkeeping_form"] == 0 and plan["reuse_throughput"] == 1 and plan["hint_passes"] == 2 and plan["kernel_timing"] == 1
    b = TW._joint(eng, objs, prm)
    b.set_observation_weights(pw, rw)
    b.run()
    full = collect(b, n_it)
    st = evidence("b", "auto_block17", shape, None, plan, b, n_it)
    assert st["ms_mlp_jac"] > 0 and st["ms_mlp_prepass"] > 0          # kernel timing arrived with the plan
    for i, o in enumerate(objs):
        m = b.debug_samples(i, o["rays"].shape[0], 50)[0]
        assert not m[rw[i] == 0].any(), "a ray of weight 0 was sampled (object %d)" % i
    b.close()
    assert full["status"].tolist() == [0] * 17
    for e in range(n_it):
        TW._check_joint_state(eng, oracle_decoder, objs, prm, oprm, pw, rw, full["trace[%d].t_obj_cam" % e], full["trace[%d].code" % e], full["trace[%d].depths" % e],
                              want={k: full["trace[%d].%s" % (e, k)] for k in ("H", "b", "dx", "V", "K")}, label="17 weighted objects, automatic plan, iteration %d" % e,
                              kind="forms/joint/auto_block17", check=(0, 8, 16), configure=_pinned("b", "auto_block17", shape, None, 1))
    for i, o in enumerate(objs):          # each object alone: wave bookkeeping, cluster tiles, the speculative band, one whole prepass launch
        c = TW._joint(eng, [o], prm)
        c.set_observation_weights([pw[i]], [rw[i]])
        c.run()
        one = collect(c, n_it)
        c.close()
        assert_same_bits("b object %d of 17 against its run alone" % i, one, {k: v[i:i + 1] for k, v in full.items()})


# ---- c. zero-weight rays equal removal ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth", [50, 64])
@pytest.mark.parametrize("form", ["block", "throughput"])
def test_c_zero_rays_equal_removal_in_the_form(eng, form, n_depth):
    def configure(b, objs):
        shape = F.shape_of(F.sizes(objs), n_depth)
        plan = F.plan_of_form(shape, form)
        assert all(plan[k] == v for k, v in F.FORMS[form]["plan"].items()), (form, plan)
        F.pin(b, F.FORMS[form]["pins"])
        return lambda b: evidence("c", "ragged3_d%d" % n_depth, shape, form, plan, b, 3)
    TW._zero_rays_equal_removal(eng, n_depth, "three_objects", configure)


# ---- d. report and posterior record, every form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape_name", ["ragged3", "detection"])
def test_d_report_in_every_form(eng, shape_name, weighted):
    objs = _objects(shape_name)
    shape = F.shape_of(F.sizes(objs))
    n_it = 3
    prm = E.gn_params(num_iterations=n_it)
    b = TW._joint(eng, objs, prm)
    pw, rw = _drawn_weights(objs, 33) if weighted else (None, None)
    if weighted:
        b.set_observation_weights(pw, rw)
    b.set_report(True)
    b.set_posterior(2, "mean")
    checked = []

    def against_the_host(form, plan):
        if form == "throughput":          # the report's rays against csrc/report_math.h on the CPU, on the sdf grid this form's pass left
            rep, rec = b.report(), b.posterior()
            n = TR._check_against_host(b, rep, rec, range(len(objs)), [(o["rays"], o["depth"]) for o in objs], 50, prm.cut_off, ray_w=rw)
            print("d %s throughput: %d rays bit-equal to the host arithmetic" % (shape_name, n))
            checked.append(n)
    ref = every_form("d", b, shape_name, shape, lambda b: (b.run(), collect(b, n_it, report=True, posterior=True, trace=False))[1], n_it + 1,
                     must_cluster=True, before=against_the_host)
    b.close()
    assert checked == [sum(o["rays"].shape[0] for o in objs)]
    assert ref["status"].tolist() == [0] * len(objs) and ref["posterior.status"].tolist() == [0] * len(objs) and (ref["report.kept_count"].sum() > 0)


# ---- e. step control with rejections -----------------------------------------------------------------------------------------------------------
STEP_FORMS = ("prepass_off", "fixed_10_passes", "block", "throughput")


def _rejected_then_accepted(dec):
    """Objects whose log holds a rejection with an accepted step behind it."""
    return [i for i in range(dec.shape[1]) if any(dec[e, i] == 2 and (dec[e + 1:, i] == 1).any() for e in range(dec.shape[0]))]


@pytest.mark.parametrize("which", ["step_control_setup", "hinted3"])
def test_e_step_control_with_rejections_in_the_hinted_and_fixed_forms(eng, which):
    n_it = SC.N
    if which == "hinted3":
        objs, prm, shape_name = F.hinted3(), E.gn_params(num_iterations=10, lr=1.0), "hinted3"
    else:
        prm = E.gn_params(num_iterations=10, lr=1.0)
        cold = ES._cold()
        objs, shape_name = cold + ES._warm_from(eng, cold, prm), "step6"
    shape = F.shape_of(F.sizes(objs))
    assert which == "hinted3" or shape == F.shape_of(F.step6_sizes())          # (the shape tests/test_feature_forms_plan.py evaluates)
    auto_plan = F.plan_of(shape)
    assert auto_plan["hint_passes"] == 2 and auto_plan["prepass_mode"] == 1          # the automatic plan: hint passes WITH the prepass
    b = ES._batch(eng, objs, prm, trace=True)
    b.set_iterations(n_it)
    b.set_step_control(*SC.DEFAULTS)
    ref = every_form("e", b, shape_name, shape, lambda b: (b.run(), collect(b, n_it, steps=True))[1], n_it, forms=STEP_FORMS)
    b.close()
    dec = ref["step_log.decision"]
    print("e %s decisions (rows = objects)\n%s\nlambdas\n%s" % (which, dec.T, ref["step_log.lambda"].T))
    assert (ref["status"] == 0).all()
    assert _rejected_then_accepted(dec), "no object of %s rejects a trial and accepts a later one" % which


# ---- f. everything on ---------------------------------------------------------------------------------------------------------------------------
def test_f_everything_on_in_every_form(eng):
    objs = F.ragged3()
    shape = F.shape_of(F.sizes(objs))
    n_it = 8
    prm = E.gn_params(num_iterations=n_it)
    b = ES._batch(eng, objs, prm, trace=True)
    b.set_observation_weights(*_drawn_weights(objs, 34))
    b.set_iterations(4)                 # the prior: the level-2 record of an earlier run (objects 0 and 2; object 1 has none)
    b.set_posterior(2, "mean")
    b.run()
    rec = b.posterior()
    assert rec["status"].tolist() == [0, 0, 0]
    b.set_iterations(n_it)
    b.set_prior(*TP._prior_of(rec, [0, 2]))
    b.set_step_control(*SC.DEFAULTS)
    live = np.ones((3, 71), np.uint8)
    live[0, [3, 5]] = 0                 # w_x, w_z of object 0, which has a prior too
    live[0, 7 + 5 * np.arange(8)] = 0   # ... and eight of its code entries
    b.set_unknowns(live)
    b.set_posterior(2, "sum")
    b.set_report(True)
    b.run()
    assert b.results()[3].tolist() == [0, 0, 0] and (b.iterations_used() == n_it).all()
    dx, sp, sc = ES._steps(b, n_it, 1.0)
    tol = ES._pick(dx, sp, sc, 1.0, lambda both, p, c: 3 <= both.min() <= n_it - 2)          # (an early stop, but not before the forms had iterations to differ in)
    assert tol is not None, "no tolerance pair stops an object early"
    b.set_convergence(tol[0], tol[1], 1)
    ref = every_form("f", b, "ragged3", shape, lambda b: (b.run(), collect(b, n_it, report=True, posterior=True, prior=True, steps=True))[1], n_it + 1, must_cluster=True)
    b.close()
    print("f: tolerances %s, iterations used %s, decisions\n%s" % (tol, ref["iterations_used"], ref["step_log.decision"].T))
    assert ref["status"].tolist() == [0, 0, 0] and 2 <= ref["iterations_used"].min() < n_it, ref["iterations_used"]
    assert np.array_equal(ref["code"][0][5 * np.arange(8)], np.zeros(8, F32)) and ref["prior.chi2"][1] == 0 and (ref["prior.chi2"][[0, 2]] > 0).all()


# ---- g. multi-view ------------------------------------------------------------------------------------------------------------------------------
def test_g_multiview_in_every_form(eng, oracle_decoder):
    objs = F.views18()
    views = [v for o in objs for v in o["views"]]
    shape = F.shape_of(F.sizes(objs), grouped=True)
    rng = np.random.default_rng(35)
    pw = [TW._weights(rng, v["pts"].shape[0]) for v in views]
    rw = [TW._weights(rng, v["rays"].shape[0]) for v in views]
    zero_views = tuple(range(3 * F.ZERO_OBJECT, 3 * F.ZERO_OBJECT + 3))
    for k in zero_views:                # every view of one object: the degenerate sums pooled by k_group_reduce
        pw[k][:] = 0
        rw[k][:] = 0
    good = [i for i in range(6) if i != F.ZERO_OBJECT]
    n_it = 3
    case = X._case(objs, n_it)
    prm, oprm = E.gn_params(num_iterations=n_it, **X.HYPER), X.oracle_params(case)
    b = eng.multiview_batch(prm, [o["t"] for o in objs], [o["views"] for o in objs], trace=True)
    b.set_observation_weights(pw, rw)
    # the unpinned run (18 members: block bookkeeping, hint passes, the mixed form) against the weighted fp64 reference, objects 0 and 5
    b.run()
    status = b.results()[3]
    print("g: status %s" % status)
    assert (status[good] == 0).all() and status[F.ZERO_OBJECT] != 0
    traces = [(b.trace(e), b.trace_views(e)) for e in range(n_it)]
    evidence("g", "views18", shape, None, F.plan_of(shape), b, n_it)
    TW._check_multiview_states(b, oracle_decoder, oprm, objs, pw, rw, traces, 50, check=(0, 5), zero_views=zero_views, label="18 weighted views, automatic plan",
                               kind="forms/multiview/views18")
    b.close()
    # weights, report, posterior, a prior from an earlier run's level-2 record, a mask on one object
    b = eng.multiview_batch(prm, [o["t"] for o in objs], [o["views"] for o in objs], trace=True)
    b.set_observation_weights(pw, rw)
    b.set_iterations(2)
    b.set_posterior(2, "mean")
    b.run()
    rec = b.posterior()
    assert (rec["status"][good] == 0).all()
    b.set_iterations(n_it)
    b.set_prior(*TP._prior_of(rec, [0, 2, 5]))
    b.set_unknowns([["translation", "scale", "code"] if i == 1 else ["all"] for i in range(6)])
    b.set_report(True)

    def run(b):
        b.run()
        return collect(b, n_it, views=True, report=True, posterior=True, prior=True)
    ref = every_form("g", b, "views18", shape, run, n_it + 1)
    auto_plan = F.plan_of(shape)
    for pins in TM.FORMS:               # the table tests/test_gpu_multiview.py pins on its two-object group, as it stands
        mine = {k[len("set_"):]: v for k, v in pins.items()}
        plan = F.plan_of(shape, mine)
        F.pin(b, mine)
        got = run(b)
        evidence("g", "views18", shape, "+".join("%s=%s" % kv for kv in pins.items()), plan, b, n_it + 1)
        F.unpin(b, mine)
        assert_same_bits("g views18 %s" % pins, got, ref, band=same_samples(plan, auto_plan))
    b.close()
    assert (ref["status"][good] == 0).all() and ref["status"][F.ZERO_OBJECT] != 0
    assert ref["report.status"][3 * F.AWAY[0] + F.AWAY[1]] == L.OBJ_FEW_SAMPLES and (ref["prior.chi2"][[0, 2, 5]] > 0).all()


# ---- h. pose-only -------------------------------------------------------------------------------------------------------------------------------
def test_h_pose_only_across_the_inlier_filter(eng):
    g = golden("golden_pose_only_8it.npz")
    n = g["pts"].shape[0]
    shape = F.shape_of(F.pose_pair_sizes(), pose_only=True)
    rng = np.random.default_rng(36)
    pw = np.concatenate([TW._weights(rng, n), TW._weights(rng, n)])
    b = eng.pose_batch(E.gn_params(pose_only_iterations=8), [g["t_co_se3"]] * 2, [float(g["scale"])] * 2, [g["pts"]] * 2, [g["code"]] * 2, trace=True)
    b.set_observation_weights(pw)
    b.set_report(True)
    b.set_posterior(2, "mean")

    def run(b):
        b.run()
        out = collect(b, 8, report=True, posterior=True)
        return {k: v for k, v in out.items() if not k.startswith("report.") or k in ("report.pt_sdf", "report.pt_flags", "report.M", "report.sum_s", "report.status")}
    ref = every_form("h", b, "pose_pair", shape, run, 8 + 1, must_cluster=True)
    b.close()
    print("h: points behind the filter %s of %d" % (ref["trace[7].K"], n))
    assert ref["status"].tolist() == [0, 0] and (ref["trace[7].K"] < n).all() and (ref["trace[4].K"] == n).all()
    assert not np.array_equal(ref["t_cam_obj"][0], ref["t_cam_obj"][1])          # (the two copies carry different weights)


# ---- i. the f16 compute mode: wave against block bookkeeping --------------------------------------------------------------------------------------
def test_i_f16_compute_mode_wave_against_block(eng):
    objs = F.ragged3()
    shape = F.shape_of(F.sizes(objs))
    n_it = 3
    b = TW._joint(eng, objs, E.gn_params(num_iterations=n_it))
    b.set_observation_weights(*_drawn_weights(objs, 37))
    b.set_report(True)
    F.pin(b, F.F16_PINS)
    out = {}
    for form in F.F16_FORMS:
        plan = F.plan_of_form(shape, form, F.F16_PINS)
        assert plan["lp_compute"] == L.COMPUTE_F16 and plan["bookkeeping_form"] == F.FORMS[form]["plan"]["bookkeeping_form"]
        F.pin(b, F.FORMS[form]["pins"])
        b.run()
        out[form] = collect(b, n_it, report=True)
        st = evidence("i", "ragged3", shape, form, plan, b, n_it + 1, compute="f16")
        assert st["n_mlp_fwd_launches"] == 0
        F.unpin(b, F.FORMS[form]["pins"])
    b.close()
    assert out["wave"]["status"].tolist() == [0, 0, 0]
    assert_same_bits("i f16 compute mode, block against wave", out["block"], out["wave"], band=True)


# ---- the record -----------------------------------------------------------------------------------------------------------------------------------
def test_worst_scaled_errors_per_form_are_printed():
    """(runs last in this file) The worst scaled fp64 errors tests b and g measured, per form, and every run's evidence, for
    profiles/feature_forms.md."""
    worst = {k[len("forms/"):]: "%.3e" % v for k, v in sorted(TW.WORST.items()) if k.startswith("forms/")}
    print("worst scaled errors against the weighted fp64 reference per form (TAU_H %.1e, TAU_B %.1e): %s" % (M.TAU_H, M.TAU_B, worst))
    print("runs with evidence: %d, forms %d" % (len(EVIDENCE), len({e["form"] for e in EVIDENCE})))
    parity_log(kind="feature_forms_worst", **{k.replace("/", "_"): v for k, v in worst.items()})
    for k in [k for k in TW.WORST if k.startswith("forms/")]:          # (tests/test_gpu_weights.py prints its own kinds)
        del TW.WORST[k]
