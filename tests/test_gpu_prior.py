"""GPU: the Gaussian prior on pose and code (dsp_batch_prior / dsp_batch_prior_fetch, include/dsp_gn.h).

  1. off and zero are exact: Lambda = 0 returns, bit for bit, everything a batch without a prior returns; in a mixed batch the objects
     without a prior keep those bits;
  2. the terms are the defined ones at every iteration: H_on - H_off = J^T Lp J and b_on - b_off = -J^T Lp e against tests/prior_ref.py,
     H_off / b_off from a batch without a prior started at the traced state -- joint, pose-only, multi-view, a 32-D decoder, the
     low-precision compute mode;
  3. a stiff prior holds the state;  4. the posterior composes;  5. the residual and chi2 at the result;  6. half a turn ends the object;
  7. the convergence rule, the partial re-run after a guard trip, and B = 1 against the same object inside a batch of four.
"""
import json

import numpy as np
import pytest

import multiview_oracle as MV
import posterior_ref as PR
import prior_ref as R
from conftest import golden
from oracle import dsp_oracle as O
from dsp_slam_amd import _lib as L, engine as E, synth

pytestmark = pytest.mark.gpu
N_IT = 10


def _bits(arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


class _Run(object):
    """All a run returns: result rows, iterations used, every trace row -- as named arrays."""

    def __init__(self, b, n_it):
        b.run()
        self.rows = b.results()
        self.used = b.iterations_used()
        self.named = list(zip(("t_cam_obj", "code", "loss", "status"), self.rows)) + [("used", self.used)]
        self.traces = [b.trace(e) for e in range(n_it)]
        for e, tr in enumerate(self.traces):
            self.named += [("%d/%s" % (e, k), tr[k]) for k in sorted(tr)]

    def bits(self, obj=None, skip_m=False):
        """skip_m: leave out the trace's m.  m counts the decoded samples with |sdf| < cut_off and is INFORMATIONAL (include/dsp_gn.h,
        dsp_compute_render_loss): with early ray termination or the prepass on, samples behind a ray's first solid sample are not decoded,
        and which ones those are follows the launch plan and the ray hints of the previous iterations -- it differs between launch forms
        and between a run and a batch restarted in its middle, with or without a prior.  Nothing that reaches a result reads it."""
        return _bits([(a if obj is None else a[obj]) for k, a in self.named if not (skip_m and k.endswith("/m"))])


def _reference_order(b, lp=False):
    """The form in which m is the reference's count: every in-sphere sample decoded, no early ray termination, no prepass (results are
    bit for bit those of every other form)."""
    b.set_ray_passes(1)
    if not lp:
        b.set_prepass(L.PREPASS_OFF)
    return b


def _joint_batch(eng, objs, prm, trace=False):
    return eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                     [o.get("code0", np.zeros(64, np.float32)) for o in objs], trace=trace)


def _prior_of(rec, keep, donor=None):
    """(t_obj_cam0, code0, Lambda) from a level-2 posterior record: objects in `keep` get their own record as the prior (pose-code cross blocks
    included), objects in `donor` = {i: j} get object j's Lambda around their OWN recorded state, everyone else Lambda = 0 (no prior)."""
    lam = np.zeros_like(rec["Lambda"])
    for i in keep:
        lam[i] = rec["Lambda"][i]
    for i, j in (donor or {}).items():
        lam[i] = rec["Lambda"][j]
    return rec["t_obj_cam"].copy(), [L.code64(c) for c in rec["code"]], lam


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ragged(eng):
    """The posterior suite's ragged batch: 64 / 120 / 250 / 300 surface points, object 1 has n_fg != M, object 3 ends DSP_OBJ_FEW_SAMPLES.
    The prior comes from ANOTHER run: the level-2 records of the same objects after 4 iterations.  Object 0 and object 2 get their own
    record, object 1 has Lambda = 0, the failing object 3 gets object 0's Lambda around its own state."""
    prm = E.gn_params(num_iterations=N_IT)
    objs = [synth.make_object(400, n_surface=64, n_background=30), synth.make_object(401, n_surface=120, n_background=40, n_foreground=90),
            synth.make_object(402, n_surface=250, n_background=200), synth.make_object(403, n_surface=300, n_background=60)]
    objs[3] = dict(objs[3], rays=np.full_like(objs[3]["rays"], np.nan))
    b = _joint_batch(eng, objs, prm)
    b.set_iterations(4)
    b.set_posterior(2, "mean")
    b.run()
    rec, status = b.posterior(), b.results()[3]
    b.close()
    assert status.tolist() == [0, 0, 0, L.OBJ_FEW_SAMPLES] and rec["status"].tolist() == [0, 0, 0, 1]
    assert np.abs(rec["Lambda"][0][:7, 7:]).max() > 0                    # the cross blocks are there
    b = _joint_batch(eng, objs, prm, trace=True)
    plain = _Run(b, N_IT)
    b.close()
    return dict(prm=prm, objs=objs, rec=rec, prior=_prior_of(rec, [0, 2], {3: 0}), plain=plain)


@pytest.fixture(scope="module")
def mixed(eng, ragged):
    """The ragged batch run with its mixed prior in its automatic forms, trace on: (the run, traces, iterations used, prior residual, level-2 record)."""
    b = _joint_batch(eng, ragged["objs"], ragged["prm"], trace=True)
    b.set_prior(*ragged["prior"])
    b.set_posterior(2, "mean")
    got = _Run(b, N_IT)
    out = dict(all=got, traces=got.traces, used=got.used, res=b.prior_residual(), rec=b.posterior())
    b.close()
    return out


# ---- 1. off and zero are exact --------------------------------------------------------------------------------------------------------------
def test_off_and_zero_are_exact(eng, ragged, mixed):
    prm, objs, plain = ragged["prm"], ragged["objs"], ragged["plain"]
    t0, z0, lam = ragged["prior"]
    b = _joint_batch(eng, objs, prm, trace=True)
    b.set_prior(t0, z0, np.zeros_like(lam))
    zero = _Run(b, N_IT)
    res = b.prior_residual()
    # ... and switched off again: the batch of before
    b.set_prior(None, None, None)
    off = _Run(b, N_IT)
    assert L.load().dsp_batch_prior_fetch(b._h, None, None) == -4              # DSP_E_STATE: the last run had no prior
    b.close()
    assert zero.bits() == plain.bits() and off.bits() == plain.bits()         # same batch, same forms: m included
    assert not res["chi2"][:3].any() and not res["e"][:3].any() and np.isnan(res["chi2"][3])
    # the mixed batch: the object with Lambda = 0 and the failing object keep the bits of the batch without a prior; the others moved
    assert mixed["all"].bits(1) == plain.bits(1)
    assert mixed["all"].rows[3].tolist() == [0, 0, 0, L.OBJ_FEW_SAMPLES] and mixed["all"].bits(3) == plain.bits(3)
    for i in (0, 2):
        assert not np.array_equal(mixed["all"].rows[0][i], plain.rows[0][i]) and not np.array_equal(mixed["all"].rows[1][i], plain.rows[1][i])


# ---- 2. the terms are the defined ones, at every iteration ----------------------------------------------------------------------------------
def _ulp32(a, b):
    return np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


def _check_terms(on_traces, used, off, prior, objects, pose_only=False, code_len=64, view_depths=None, what="", auto_traces=None):
    """For every traced iteration e of the prior-on run: the batch `off` (no prior, one iteration, trace on) is started at the traced state;
    |H_on - H_off - J^T Lp J| and |b_on - b_off + J^T Lp e| stay within 2 float32 ulps of the larger of the two traced entries (both are fp64
    values rounded once to float32), V, m and K are identical.  Both batches run in _reference_order, the form in which m is a defined
    quantity (_Run.bits); auto_traces: the same prior-on run in its automatic forms -- H, b, dx, V, K and the states are bit for bit the
    same, its m is at most the reference's."""
    t0, z0, lam = prior
    worst_h = worst_b = 0.0
    for e, tr in enumerate(on_traces):
        if auto_traces is not None:
            for i in [i for i in objects if e < used[i]]:
                for k in ("H", "b", "dx", "V", "K", "t_obj_cam", "code", "depths"):
                    assert np.array_equal(auto_traces[e][k][i], tr[k][i]), (what, "automatic forms", k, e, i)
                assert auto_traces[e]["m"][i] <= tr["m"][i]
        live = [i for i in objects if e < used[i]]
        if not live:
            continue
        if pose_only:
            off.set_start_state(tr["t_obj_cam"])
        else:
            off.set_start_state(tr["t_obj_cam"], tr["code"], tr["depths"] if view_depths is None else view_depths[e])
        off.run()
        t1 = off.trace(0)
        for i in live:
            assert np.array_equal(t1["t_obj_cam"][i], tr["t_obj_cam"][i])
            assert (t1["V"][i], t1["m"][i], t1["K"][i]) == (tr["V"][i], tr["m"][i], tr["K"][i]), (what, e, i)
            ref = R.terms(tr["t_obj_cam"][i], tr["code"][i], t0[i], z0[i], lam[i], pose_only, code_len)
            h_on, h_off = tr["H"][i].astype(np.float64), t1["H"][i].astype(np.float64)
            b_on, b_off = tr["b"][i].astype(np.float64), t1["b"][i].astype(np.float64)
            eh = np.abs(h_on - h_off - ref["H"]) / _ulp32(h_on, h_off)
            eb = np.abs(b_on - b_off - ref["b"]) / _ulp32(b_on, b_off)
            worst_h, worst_b = max(worst_h, eh.max()), max(worst_b, eb.max())
            assert eh.max() <= 2.0, (what, e, i, eh.max())
            assert eb.max() <= 2.0, (what, e, i, eb.max())
    print("%s: worst |H_on - H_off - J^T Lp J| = %.2f ulp, worst |b_on - b_off + J^T Lp e| = %.2f ulp" % (what, worst_h, worst_b))
    return worst_h, worst_b


def test_terms_joint(eng, ragged, mixed):
    on = _reference_order(_joint_batch(eng, ragged["objs"], ragged["prm"], trace=True))
    on.set_prior(*ragged["prior"])
    full = _Run(on, N_IT)
    on.close()
    off = _reference_order(_joint_batch(eng, ragged["objs"], ragged["prm"], trace=True))
    off.set_iterations(1)
    assert mixed["used"][:3].tolist() == [N_IT] * 3 and _bits(full.rows) == _bits(mixed["all"].rows) and np.array_equal(full.used, mixed["used"])
    _check_terms(full.traces, full.used, off, ragged["prior"], [0, 2], what="joint B = 4", auto_traces=mixed["traces"])
    off.close()


def test_terms_low_precision_compute(eng, ragged):
    """The low-precision compute mode runs with a prior, and check 2 holds in it (both batches in the mode)."""
    def make():
        b = _joint_batch(eng, ragged["objs"][:3], ragged["prm"], trace=True)
        b.set_compute(L.COMPUTE_F16)
        b.set_lp_small_batches(1)
        return _reference_order(b, lp=True)
    t0, z0, lam = ragged["prior"]
    prior = (t0[:3], z0[:3], lam[:3])
    on = make()
    on.set_prior(*prior)
    on.run()
    traces, used, status = [on.trace(e) for e in range(N_IT)], on.iterations_used(), on.results()[3]
    on.close()
    assert status.tolist() == [0, 0, 0]
    off = make()
    off.set_iterations(1)
    _check_terms(traces, used, off, prior, [0, 2], what="f16 compute mode")
    off.close()


def _pose_objects():
    g, g5 = golden("golden_pose_only_8it.npz"), golden("golden_pose_only.npz")
    return [(g["t_co_se3"], float(g["scale"]), g["pts"], g["code"]), (g5["t_co_se3"], float(g5["scale"]), g5["pts"][:200], g5["code"])]


def _pose_batch(eng, objs, n_it, trace=False):
    return eng.pose_batch(E.gn_params(pose_only_iterations=n_it), [o[0] for o in objs], [o[1] for o in objs], [o[2] for o in objs], [o[3] for o in objs], trace=trace)


@pytest.fixture(scope="module")
def pose_case(eng):
    """Two pose-only objects (the first has planted outliers: the inlier filter of iteration 4 drops points), 8 iterations; the prior is the
    level-2 record of a 3-iteration run of the same objects."""
    objs = _pose_objects()
    b = _pose_batch(eng, objs, 3)
    b.set_posterior(2, "mean")
    b.run()
    rec = b.posterior()
    b.close()
    assert rec["status"].tolist() == [0, 0]
    prior = (rec["t_obj_cam"].copy(), None, rec["Lambda"][:, :6, :6].copy())
    on = _pose_batch(eng, objs, 8, trace=True)
    on.set_prior(*prior)
    on.set_posterior(2, "mean")
    on.run()
    out = dict(objs=objs, prior=prior, traces=[on.trace(e) for e in range(8)], used=on.iterations_used(), rows=on.results(), res=on.prior_residual(),
               rec=on.posterior())
    on.close()
    return out


def test_terms_pose_only(eng, oracle_decoder, pose_case):
    objs, prior, traces = pose_case["objs"], pose_case["prior"], pose_case["traces"]
    assert pose_case["rows"][3].tolist() == [0, 0] and pose_case["used"].tolist() == [8, 8]
    # iterations 0 .. 4 are built from every point: a batch without a prior restarted at the traced state has the same system
    off = _pose_batch(eng, objs, 1, trace=True)
    z = np.zeros((2, 64), np.float32)
    _check_terms([dict(tr, code=z) for tr in traces[:5]], [5, 5], off, (prior[0], z, prior[2]), [0, 1], pose_only=True, what="pose-only, iterations 0 .. 4")
    off.close()
    # iterations 5 .. 7 are built from the points the inlier filter kept (|sdf| <= 0.05 at the start of iteration 4), which no restarted batch
    # reproduces: the system without the prior is the oracle's float32 one on those points.  Bound: 1e-4 of the largest entry, the bound
    # tests/test_gpu_posterior.py::test_filtered_pose_only_set holds the same comparison to (b: of the largest sum of absolute terms).
    k4 = [int(k) for k in traces[4]["K"]]
    assert int(traces[5]["K"][0]) < k4[0] == 300, "the inlier filter did not run"
    for i in (0, 1):
        pts, code = objs[i][2], objs[i][3]
        keep = np.abs(O.pose_only_system(oracle_decoder, pts, traces[4]["t_obj_cam"][i], code)["res"]) <= O.POSE_INLIER_TH
        for e in (5, 6, 7):
            tr = traces[e]
            assert int(tr["K"][i]) == int(keep.sum())
            sysm = O.pose_only_system(oracle_decoder, pts[keep], tr["t_obj_cam"][i], code)
            ref = R.terms(tr["t_obj_cam"][i], None, prior[0][i], None, prior[2][i], pose_only=True)
            j7, _, res = O.compute_sdf_loss(oracle_decoder, np.asarray(pts[keep], np.float32), tr["t_obj_cam"][i], np.asarray(code, np.float32))
            scale_b = (np.abs(np.asarray(j7, np.float64)[:, :6]).T @ np.abs(np.asarray(res, np.float64).reshape(-1))).max() / keep.sum()
            eh = np.abs(tr["H"][i].astype(np.float64) - sysm["H"] - ref["H"]).max() / np.abs(sysm["H"]).max()
            eb = np.abs(tr["b"][i].astype(np.float64) - sysm["b"] - ref["b"]).max() / scale_b
            print("pose-only past the filter: object %d iteration %d K %d: H %.2e b %.2e" % (i, e, tr["K"][i], eh, eb))
            assert eh <= 1e-4 and eb <= 1e-4


@pytest.fixture(scope="module")
def mv_case(eng):
    """golden_multiview_cars3 (3 views); the prior is the level-2 record of a 3-iteration run."""
    g = golden("golden_multiview_cars3.npz")
    cfg = json.loads(str(g["cfg_json"]))
    prm = E.params_from_configs(cfg)
    n_it = int(g["it_H"].shape[0])

    def make(trace=False):
        return eng.multiview_batch(prm, [g["in_t_cam_obj_init"]], [MV.golden_views(g)], trace=trace)
    b = make()
    b.set_iterations(3)
    b.set_posterior(2, "sum")
    b.run()
    rec = b.posterior()
    b.close()
    assert rec["status"].tolist() == [0]
    return dict(make=make, n_it=n_it, prior=_prior_of(rec, [0]), cfg=cfg)


def test_terms_multiview(mv_case):
    make, n_it, prior = mv_case["make"], mv_case["n_it"], mv_case["prior"]
    auto = make(trace=True)
    auto.set_prior(*prior)
    auto_run = _Run(auto, n_it)
    auto.close()
    on = _reference_order(make(trace=True))
    on.set_prior(*prior)
    on.run()
    traces, views, used, status = [on.trace(e) for e in range(n_it)], [on.trace_views(e) for e in range(n_it)], on.iterations_used(), on.results()[3]
    assert _bits(on.results()) == _bits(auto_run.rows)
    on.close()
    assert status.tolist() == [0] and used.tolist() == [n_it]
    off = _reference_order(make(trace=True))
    off.set_iterations(1)
    _check_terms(traces, used, off, prior, [0], view_depths=[v["depths"] for v in views], what="multi-view, 3 views (the leader's row)",
                 auto_traces=auto_run.traces)
    off.close()


def test_terms_32d_decoder(chairs32_decoder):
    """The chairs32 decoder, once: slots beyond the code length carry no prior, and their rows stay pinned to the identity."""
    g = golden("golden_recon_chairs32.npz")
    cfg = json.loads(str(g["cfg_json"]))
    prm = E.params_from_configs(cfg)
    n_it = int(g["it_H"].shape[0])
    e32 = E.Engine(chairs32_decoder.layers, chairs32_decoder.latent_in, chairs32_decoder.code_len, device=0)
    try:
        def make():
            return e32.batch(prm, [g["in_t_cam_obj_init"]], [g["in_pts"]], [g["in_rays"]], [g["in_depth"]], [g["in_code"]] if "in_code" in g.files else None, trace=True)
        b = make()
        b.set_iterations(3)
        b.set_posterior(2, "mean")
        b.run()
        rec = b.posterior()
        assert rec["status"].tolist() == [0] and not rec["Lambda"][0][39:].any()
        prior = _prior_of(rec, [0])
        bad = prior[2].copy()
        bad[0, 50, 50] = 1.0
        assert L.load().dsp_batch_prior(b._h, L.ptr(L.f32(prior[0])), L.ptr(L.f32(np.stack(prior[1]))), L.ptr(bad, L.c_f64p)) == -1       # beyond the code length
        b.close()
        auto = make()
        auto.set_prior(*prior)
        auto_run = _Run(auto, n_it)
        auto.close()
        on = _reference_order(make())
        on.set_prior(*prior)
        on.run()
        traces, used = [on.trace(e) for e in range(n_it)], on.iterations_used()
        assert on.results()[3].tolist() == [0] and _bits(on.results()) == _bits(auto_run.rows)
        on.close()
        for tr in traces:
            h = tr["H"][0]
            assert np.array_equal(h[39:, 39:], np.eye(32, dtype=np.float32)) and not h[:39, 39:].any() and not tr["b"][0][39:].any() and not tr["dx"][0][39:].any()
        off = _reference_order(make())
        off.set_iterations(1)
        _check_terms(traces, used, off, prior, [0], code_len=32, what="chairs32", auto_traces=auto_run.traces)
        off.close()
    finally:
        e32.close()


# ---- 3. a stiff prior holds the state ------------------------------------------------------------------------------------------------------
def test_stiff_prior_holds_the_state(eng, ragged):
    """Lp = lambda I on the used slots, lambda = 1e10, centred on the start state: H - lambda J^T J is positive semi-definite and J = I at
    e = 0, so every step obeys |dx| <= |b| / lambda (b the traced total; 1e-6 covers the float32 rounding of the traced b and dx)."""
    lam_v = 1e10
    objs, prm, plain = ragged["objs"][:3], ragged["prm"], ragged["plain"]
    t_start = plain.traces[0]["t_obj_cam"][:3]
    b = _joint_batch(eng, objs, prm, trace=True)
    b.set_prior(t_start, np.zeros((3, 64), np.float32), np.stack([lam_v * np.eye(71)] * 3))
    b.run()
    assert b.results()[3].tolist() == [0, 0, 0]
    for e in range(N_IT):
        tr = b.trace(e)
        for i in range(3):
            nd, nb = np.linalg.norm(tr["dx"][i].astype(np.float64)), np.linalg.norm(tr["b"][i].astype(np.float64))
            assert nd <= nb / lam_v * (1 + 1e-6), (e, i, nd, nb / lam_v)
    res = b.prior_residual()
    assert np.abs(res["e"]).max() < 1e-4       # the state is float32: ten roundings of entries up to ~10
    b.close()
    # pose-only, past the inlier filter
    po = _pose_objects()
    p = _pose_batch(eng, po, 8, trace=True)
    p.run()
    t_start = p.trace(0)["t_obj_cam"]
    p.set_prior(t_start, None, np.stack([lam_v * np.eye(6)] * 2))
    p.run()
    assert p.results()[3].tolist() == [0, 0]
    for e in range(8):
        tr = p.trace(e)
        for i in range(2):
            nd, nb = np.linalg.norm(tr["dx"][i].astype(np.float64)), np.linalg.norm(tr["b"][i].astype(np.float64))
            assert nd <= nb / lam_v * (1 + 1e-6), (e, i, nd, nb / lam_v)
    p.close()


# ---- 4. the posterior composes ---------------------------------------------------------------------------------------------------------------
def test_posterior_composes_joint(eng, ragged, mixed):
    """With a prior on, the level-2 record is the linearisation of a batch with the same prior started at the record's state: float32(Lambda +
    damping) and float32(g) are that batch's traced H and b, bit for bit; the result rows do not depend on the posterior being on."""
    prm, objs, rec = ragged["prm"], ragged["objs"], mixed["rec"]
    b = _joint_batch(eng, objs, prm, trace=True)
    b.set_prior(*ragged["prior"])
    rows_without = _Run(b, N_IT)                              # the posterior off
    assert rows_without.bits() == mixed["all"].bits()
    b.set_start_state(rec["t_obj_cam"], [L.code64(c) for c in rec["code"]])
    b.set_iterations(1)
    b.run()
    tr = b.trace(0)
    b.close()
    assert rec["status"].tolist() == [0, 0, 0, 1]
    for i in range(3):
        h = PR.with_damping(rec["Lambda"][i], prm.s_damp, 64).astype(np.float32)
        assert np.array_equal(h, tr["H"][i]) and np.array_equal(rec["g"][i].astype(np.float32), tr["b"][i]), i
    # the record with the prior is the record without it plus the prior's block (object 0; object 1 has no prior: the same record)
    assert np.abs(rec["Lambda"][0] - ragged["rec"]["Lambda"][0]).max() > 0


def test_posterior_composes_pose_only_and_multiview(eng, pose_case, mv_case):
    objs, prior = pose_case["objs"], pose_case["prior"]
    # pose-only, 3 iterations: every point is still alive, so a restarted batch has the record's system
    b = _pose_batch(eng, objs, 3, trace=True)
    b.set_prior(*prior)
    b.set_posterior(2, "mean")
    b.run()
    rec, rows = b.posterior(), b.results()
    b.set_posterior(0)
    b.run()
    assert _bits(b.results()) == _bits(rows)
    b.set_start_state(rec["t_obj_cam"])
    b.set_iterations(1)
    b.run()
    tr = b.trace(0)
    b.close()
    for i in range(2):
        assert np.array_equal(PR.with_damping(rec["Lambda"][i][:6, :6], 0.0, 64, True).astype(np.float32), tr["H"][i])
        assert np.array_equal(rec["g"][i][:6].astype(np.float32), tr["b"][i])
    # multi-view
    make, cfg = mv_case["make"], mv_case["cfg"]
    m = make(trace=True)
    m.set_prior(*mv_case["prior"])
    m.set_posterior(2, "mean")
    m.run()
    rec, rows = m.posterior(), m.results()
    m.set_posterior(0)
    m.run()
    assert _bits(m.results()) == _bits(rows)
    m.set_start_state(rec["t_obj_cam"], [L.code64(c) for c in rec["code"]])
    m.set_iterations(1)
    m.run()
    tr = m.trace(0)
    m.close()
    assert rec["status"].tolist() == [0]
    h = PR.with_damping(rec["Lambda"][0], cfg["optimizer"]["joint_optim"]["scale_damping"], 64).astype(np.float32)
    assert np.array_equal(h, tr["H"][0]) and np.array_equal(rec["g"][0].astype(np.float32), tr["b"][0])


# ---- 5. the residual at the result ---------------------------------------------------------------------------------------------------------
def test_residual_at_the_result(ragged, mixed, pose_case):
    """prior_residual() against prior_ref at the RETURNED state: 1e-9 absolute on e, 1e-9 relative on chi2.  The state is read from the
    level-2 record of the same run (the camera -> object matrix the device holds, bit for bit; the result row carries its float32 INVERSE,
    from which e is recovered only to ~1e-6, checked as well)."""
    t0, z0, lam = ragged["prior"]
    res, rec, rows = mixed["res"], mixed["rec"], mixed["all"].rows
    for i in (0, 2):
        ref = R.terms(rec["t_obj_cam"][i], L.code64(rec["code"][i]), t0[i], z0[i], lam[i])
        assert np.abs(res["e"][i] - ref["e"]).max() <= 1e-9 and abs(res["chi2"][i] - ref["chi2"]) <= 1e-9 * ref["chi2"]
        assert np.array_equal(rec["code"][i], rows[1][i])
        from_row = R.terms(np.linalg.inv(rows[0][i].astype(np.float64)), rows[1][i], t0[i], z0[i], lam[i])
        assert np.abs(res["e"][i] - from_row["e"]).max() <= 1e-5
        print("object %d: chi2 %.4g, |e_pose| %.3g, |e_code| %.3g" % (i, res["chi2"][i], np.linalg.norm(res["e"][i][:7]), np.linalg.norm(res["e"][i][7:])))
    assert res["chi2"][1] == 0 and not res["e"][1].any()                       # no prior
    assert np.isnan(res["chi2"][3]) and np.isnan(res["e"][3]).all()            # did not end good
    # pose-only: e has 6 entries, chi2 against the 6 x 6 Lambda
    pres, prec, prior = pose_case["res"], pose_case["rec"], pose_case["prior"]
    assert pres["e"].shape == (2, 6)
    for i in range(2):
        ref = R.terms(prec["t_obj_cam"][i], None, prior[0][i], None, prior[2][i], pose_only=True)
        assert np.abs(pres["e"][i] - ref["e"]).max() <= 1e-9 and abs(pres["chi2"][i] - ref["chi2"]) <= 1e-9 * ref["chi2"]


# ---- 6. half a turn --------------------------------------------------------------------------------------------------------------------------
def test_half_a_turn(eng, ragged, mixed):
    """T0 = the start pose rotated by pi about y: T_oc T0^-1 is half a turn, the object ends DSP_OBJ_NAN; its neighbours keep their bits."""
    prm, objs = ragged["prm"], ragged["objs"]
    t0, z0, lam = (np.array(a, copy=True) for a in ragged["prior"])
    start = ragged["plain"].traces[0]["t_obj_cam"]
    t0[0] = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ start[0].astype(np.float64)).astype(np.float32)
    b = _joint_batch(eng, objs, prm, trace=True)
    b.set_prior(t0, z0, lam)
    got = _Run(b, N_IT)
    res = b.prior_residual()
    b.close()
    assert got.rows[3].tolist() == [L.OBJ_NAN, 0, 0, L.OBJ_FEW_SAMPLES] and got.used[0] == 0
    assert np.isnan(res["chi2"][0]) and np.isnan(res["e"][0]).all()
    for i in (1, 2):
        assert got.bits(i) == mixed["all"].bits(i)
    assert res["chi2"][2] == mixed["res"]["chi2"][2]


# ---- 7. bit-equality across forms and modes ------------------------------------------------------------------------------------------------
def _pick_rule(traces, good, n_it):
    """A rule (tol, tol, 1) that freezes at least one good object before the last iteration, with every step at least 5 % away from it."""
    dx = np.stack([tr["dx"] for tr in traces]).astype(np.float64)[:, good]
    sp, sc = np.abs(dx[:, :, :7]).max(-1), np.abs(dx[:, :, 7:]).max(-1)
    for tol in np.geomspace(1e-4, 10.0, 41):
        steps = np.concatenate([sp.ravel(), sc.ravel()])
        if np.any((steps > tol / 1.05) & (steps < tol * 1.05)):
            continue
        if np.any((sp[:-1] < tol) & (sc[:-1] < tol)):
            return float(tol), float(tol), 1
    raise AssertionError("no tolerance of the grid freezes an object of this batch early")


def test_convergence_rule_with_a_prior(eng, ragged, mixed):
    """A frozen object equals the shorter run with the same prior, bit for bit (the prior's terms stop with it)."""
    prm, objs = ragged["prm"], ragged["objs"]
    lr = prm.lr
    scaled = [dict(tr, dx=tr["dx"] * lr) for tr in mixed["traces"]]
    rule = _pick_rule(scaled, [0, 1, 2], N_IT)
    b = _joint_batch(eng, objs, prm)
    b.set_prior(*ragged["prior"])
    b.set_convergence(*rule)
    b.run()
    rows, used, res = b.results(), b.iterations_used(), b.prior_residual()
    b.set_convergence(0.0, 0.0, 1)
    print("rule", rule, "iterations used", used)
    assert used[:3].min() < N_IT and rows[3].tolist() == [0, 0, 0, L.OBJ_FEW_SAMPLES]
    for n in sorted(set(int(u) for u in used[:3])):
        b.set_iterations(n)
        b.run()
        short, sres = b.results(), b.prior_residual()
        for i in range(3):
            if used[i] == n:
                assert _bits([a[i] for a in short]) == _bits([a[i] for a in rows]), (i, n)
                assert sres["chi2"][i] == res["chi2"][i] and np.array_equal(sres["e"][i], res["e"][i])
    b.close()


def test_partial_rerun_keeps_the_prior(oracle_decoder, ragged):
    """A forced bf16 margin of 2e-5 trips the prepass guard: the tripped objects run again with the prepass off AND the prior; rows and
    residuals are the prepass-off run's, bit for bit."""
    prm, objs = ragged["prm"], ragged["objs"]
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    out = {}
    for name, mode, delta in (("off", L.PREPASS_OFF, -1.0), ("trip", L.PREPASS_BF16, 2e-5)):
        b = _joint_batch(own, objs, prm)
        b.set_prepass(mode, delta)
        b.set_prior(*ragged["prior"])
        b.run()
        out[name] = (b.results(), b.prior_residual(), b.stats())
        b.close()
    own.close()
    st = out["trip"][2]
    print("guard trips", st["prepass_guard_trips"], "objects re-run", st["prepass_guard_objects"])
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_trips"] > 0
    assert _bits(out["trip"][0]) == _bits(out["off"][0])
    assert _bits([out["trip"][1]["e"], out["trip"][1]["chi2"]]) == _bits([out["off"][1]["e"], out["off"][1]["chi2"]])


def test_one_object_alone_equals_the_batch(eng, ragged, mixed):
    """B = 1 in its automatic forms (direct tiles, cluster form, speculative band) equals the same object inside the batch of four."""
    prm, objs = ragged["prm"], ragged["objs"]
    t0, z0, lam = ragged["prior"]
    for i in (0, 2):
        b = _joint_batch(eng, [objs[i]], prm, trace=True)
        b.set_prior(t0[i:i + 1], z0[i:i + 1], lam[i:i + 1])
        alone = _Run(b, N_IT)
        res = b.prior_residual()
        b.close()
        assert alone.bits(0, skip_m=True) == mixed["all"].bits(i, skip_m=True), i          # (other launch forms: m is not comparable, _Run.bits)
        assert res["chi2"][0] == mixed["res"]["chi2"][i] and np.array_equal(res["e"][0], mixed["res"]["e"][i])
