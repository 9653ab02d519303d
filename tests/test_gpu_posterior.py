"""GPU: the posterior pass (dsp_batch_posterior / dsp_batch_posterior_fetch, include/dsp_gn.h) -- one more linearisation at the state the run
returns, turned into pose information / covariance and code variance per object.

  * results untouched: pose, code, loss, status, iterations used and every trace row are bit-equal with the posterior off, at level 1 and at
    level 2 -- joint (ragged, one failing object, with and without a convergence rule that freezes some), pose-only and multi-view batches;
  * the record IS the iteration's own linearisation: a second batch started at the record's state reproduces float32(Lambda + damping) and
    float32(g) in its trace bit for bit, V, K and the loss likewise -- so the record inherits what the suite pins about the trace's H;
  * the filtered pose-only set, SUM weights, the inverse against a refined fp64 / long double reference, the singular flag, independence of
    objects, the path through Optimizer / pose_graph / tools/reoptimise_map.py, and the low-precision compute mode.
"""
import json
import os
import sys

import numpy as np
import pytest

import forensics as F
import gn_metric as M
import multiview_oracle as MV
import posterior_ref as R
from conftest import ROOT, golden
from oracle import dsp_oracle as O
from dsp_slam_amd import _lib as L, engine as E, fixtures, pose_graph as P, synth
from dsp_slam_amd.map_objects import write_map_objects

pytestmark = pytest.mark.gpu
N_IT = 10
OK, NONE, SINGULAR = L.POSTERIOR_OK, L.POSTERIOR_NONE, L.POSTERIOR_SINGULAR
L1_KEYS = ("status", "info_pose", "cov_pose", "var_code", "loss", "M", "V", "K")


class _Engines(object):
    def __init__(self, decoders):
        self.decoders, self.engines = decoders, {}

    def __call__(self, code_len=64):
        if code_len not in self.engines:
            d = self.decoders[code_len]
            self.engines[code_len] = E.Engine(d.layers, d.latent_in, d.code_len, device=0)
        return self.engines[code_len], self.decoders[code_len]

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def engines(oracle_decoder, chairs32_decoder):
    es = _Engines({64: oracle_decoder, 32: chairs32_decoder})
    yield es
    es.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines(64)[0]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _same_record(a, b, i, j, keys=L1_KEYS):
    return all(np.array_equal(a[k][i], b[k][j], equal_nan=True) for k in keys)


def _sym(a):
    return np.array_equal(a, np.swapaxes(a, -1, -2))


def _joint_batch(eng, objs, prm, trace=False):
    return eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                     [o.get("code0", np.zeros(64, np.float32)) for o in objs], trace=trace)


def _everything(b, n_it, views=False):
    """All a run returns: result rows, iterations used, every trace row."""
    b.run()
    out = list(b.results()) + [b.iterations_used()]
    for e in range(n_it):
        tr = b.trace(e)
        out += [tr[k] for k in sorted(tr)]
        if views:
            tv = b.trace_views(e)
            out += [tv[k] for k in sorted(tv)]
    return out


def _across_levels(make, n_it, rule=None, views=False):
    """The batch run with the posterior off, at level 1 and at level 2: everything bit-equal -> (rows of level 0, record of level 1, of level 2)."""
    got, recs = [], []
    for level in (0, 1, 2):
        b = make()
        if rule is not None:
            b.set_convergence(*rule)
        b.set_posterior(level, "mean")
        got.append(_everything(b, n_it, views))
        if level == 0:
            assert L.load().dsp_batch_posterior_fetch(b._h, *([None] * 13)) == -4            # DSP_E_STATE: no run with the posterior on
        else:
            recs.append(b.posterior())
        b.close()
    assert _same(got[0], got[1]) and _same(got[0], got[2])
    assert "Lambda" not in recs[0] and recs[1]["Lambda"].shape[1:] == (71, 71)
    assert _same_record(recs[0], recs[1], slice(None), slice(None))                                 # level 2 adds fields, changes none
    return got[0], recs[0], recs[1]


def _pick_rule(make, n_it, good, pose_only=False):
    """A convergence rule (tol, tol, 1) that freezes at least one of the `good` objects before the last iteration, read off a traced, unstopped
    run: the smallest tolerance of a fixed grid that does, with every step of every object at least 5 % away from it (the device compares
    the fp64 step, the trace holds it in fp32)."""
    b = make()
    b.run()
    dx = np.stack([b.trace(e)["dx"] for e in range(n_it)]).astype(np.float64)[:, good]
    b.close()
    p = 6 if pose_only else 7
    sp = np.abs(dx[:, :, :p]).max(-1)
    sc = np.zeros_like(sp) if pose_only else np.abs(dx[:, :, p:]).max(-1)
    for tol in np.geomspace(1e-4, 10.0, 41):
        steps = np.concatenate([sp.ravel(), sc.ravel()])
        if np.any((steps > tol / 1.05) & (steps < tol * 1.05)):
            continue
        if np.any((sp[:-1] < tol) & (sc[:-1] < tol)):
            return float(tol), float(tol), 1
    raise AssertionError("no tolerance of the grid freezes an object of this batch early")


@pytest.fixture(scope="module")
def ragged(eng):
    """64 / 120 / 250 / 300 surface points; object 1 has n_fg != M; object 3 ends DSP_OBJ_FEW_SAMPLES (no ray reaches the sphere); objects 0
    and 1 are warm-started from their own results, so that a convergence rule freezes them early."""
    prm = E.gn_params(num_iterations=N_IT)
    objs = [synth.make_object(400, n_surface=64, n_background=30), synth.make_object(401, n_surface=120, n_background=40, n_foreground=90),
            synth.make_object(402, n_surface=250, n_background=200), synth.make_object(403, n_surface=300, n_background=60)]
    objs[3] = dict(objs[3], rays=np.full_like(objs[3]["rays"], np.nan))
    b = _joint_batch(eng, objs, prm)
    b.run()
    t, code, _, status = b.results()
    b.close()
    assert status.tolist() == [0, 0, 0, L.OBJ_FEW_SAMPLES]
    for i in (0, 1):
        objs[i] = dict(objs[i], t_cam_obj_init=t[i].copy(), code0=L.code64(code[i]))
    return prm, objs


def test_results_untouched_joint(eng, ragged):
    prm, objs = ragged
    for rule in (None, _pick_rule(lambda: _joint_batch(eng, objs, prm, trace=True), N_IT, [0, 1, 2])):
        rows, rec1, rec2 = _across_levels(lambda: _joint_batch(eng, objs, prm, trace=True), N_IT, rule)
        used = rows[4]
        print("rule", rule, "iterations used", used, "posterior status", rec1["status"], "M V K", rec1["M"], rec1["V"], rec1["K"])
        assert rows[3].tolist() == [0, 0, 0, L.OBJ_FEW_SAMPLES]
        assert rec1["status"].tolist() == [OK, OK, OK, NONE]
        if rule is not None:
            assert used[:3].min() < N_IT, used            # some objects froze early, and they have a record
        for rec in (rec1, rec2):
            assert _sym(rec["info_pose"]) and _sym(rec["cov_pose"])
            assert not rec["cov_pose"][3].any() and not rec["var_code"][3].any() and not rec["info_pose"][3].any()
            assert (rec["M"][:3] == [64, 120, 250]).all() and (rec["K"][:3] > 0).all() and (rec["V"][:3] >= 10).all()
        assert _sym(rec2["Lambda"])


def _pose_objects():
    g, g5 = golden("golden_pose_only_8it.npz"), golden("golden_pose_only.npz")
    return [(g["t_co_se3"], float(g["scale"]), g["pts"], g["code"]), (g5["t_co_se3"], float(g5["scale"]), g5["pts"][:200], g5["code"]),
            (g["allout_t_co_se3"], float(g["allout_scale"]), g["allout_pts"], g["allout_code"])]


def _pose_batch(eng, objs, n_it, trace=False):
    return eng.pose_batch(E.gn_params(pose_only_iterations=n_it), [o[0] for o in objs], [o[1] for o in objs], [o[2] for o in objs], [o[3] for o in objs], trace=trace)


def test_results_untouched_pose_only(eng):
    objs = _pose_objects()               # the third loses every point to the inlier filter: NaN like the reference's, no record
    for rule in (None, _pick_rule(lambda: _pose_batch(eng, objs, 8, trace=True), 8, [0, 1], pose_only=True)):
        rows, rec1, rec2 = _across_levels(lambda: _pose_batch(eng, objs, 8, trace=True), 8, rule)
        print("pose-only: rule", rule, "used", rows[4], "status", rec1["status"], "M", rec1["M"])
        assert rows[3].tolist() == [0, 0, L.OBJ_NAN] and rec1["status"].tolist() == [OK, OK, NONE]
        if rule is not None:
            assert rows[4][:2].min() < 8, rows[4]
        assert rec1["info_pose"].shape == (3, 6, 6) and _sym(rec1["info_pose"]) and _sym(rec1["cov_pose"]) and not rec1["var_code"].any()
        assert np.array_equal(rec2["Lambda"][:, :6, :6], rec2["info_pose"]) and not rec2["Lambda"][:, 6:].any() and not rec2["Lambda"][:, :, 6:].any()


def test_results_untouched_multiview(eng):
    prm = E.gn_params(num_iterations=6)
    o3, o2 = synth.make_object_multiview(21, n_views=3, n_surface=120, n_background=40), synth.make_object_multiview(22, n_views=2, n_surface=120, n_background=40)
    o1 = synth.make_object(404, n_surface=150, n_background=40)
    t0 = [o3["t_cam_obj_init"], o1["t_cam_obj_init"], o2["t_cam_obj_init"]]
    views = [o3["views"], [dict(t_ref_cam=np.eye(4, dtype=np.float32), pts=o1["pts"], rays=o1["rays"], depth=o1["depth"])], o2["views"]]
    codes = [np.zeros(64, np.float32)] * 3
    mv = eng.multiview_batch(prm, t0, views, codes)
    mv.run()
    t, code, _, status = mv.results()
    mv.close()
    assert (status == 0).all()
    t0, views, codes = t0 + [t[0].copy()], views + [o3["views"]], codes + [L.code64(code[0])]          # the three-view object again, warm: it freezes first
    unstopped = None
    for rule in (None, _pick_rule(lambda: eng.multiview_batch(prm, t0, views, codes, trace=True), 6, [0, 1, 2, 3])):
        rows, rec1, rec2 = _across_levels(lambda: eng.multiview_batch(prm, t0, views, codes, trace=True), 6, rule, views=True)
        unstopped = rec2 if rule is None else unstopped
        print("multi-view: rule", rule, "used", rows[4], "status", rec1["status"], "M V K", rec1["M"], rec1["V"], rec1["K"])
        assert (rows[3] == 0).all() and (rec1["status"] == OK).all() and rec1["status"].shape == (4,)          # per object, not per view
        assert rec1["M"].tolist() == [360, 150, 240, 360]
        if rule is not None:
            assert rows[4].min() < 6, rows[4]
    # one view IS the single-view batch: the same record, bit for bit
    b = _joint_batch(eng, [o1], prm)
    b.set_posterior(2, "mean")
    b.run()
    single = b.posterior()
    b.close()
    assert _same_record(single, unstopped, 0, 1, L1_KEYS + ("Lambda", "g", "t_obj_cam", "code", "depths"))


# ---- the chain to the reference -----------------------------------------------------------------------------------------------------------
CHAIN = ["golden_recon_small.npz", "golden_recon_freiburg.npz", "golden_recon_chairs32.npz", "golden_multiview_cars3.npz", "golden_pose_only.npz"]
_RECORDS = {}


def _golden_batch(engines, name, trace=False):
    """(batch of the golden's inputs, cfg, oracle params, decoder, code_len, iterations)."""
    g = golden(name)
    if name == "golden_pose_only.npz":
        e, dec = engines(64)
        b = e.pose_batch(E.gn_params(pose_only_iterations=3), [g["t_co_se3"]], [float(g["scale"])], [g["pts"]], [g["code"]], trace=trace)
        return b, None, None, dec, 64, 3
    cfg = json.loads(str(g["cfg_json"]))
    prm, oprm = E.params_from_configs(cfg), O.GNParams.from_configs(cfg)
    e, dec = engines(cfg["optimizer"]["code_len"])
    if name.startswith("golden_multiview"):
        b = e.multiview_batch(prm, [g["in_t_cam_obj_init"]], [MV.golden_views(g)], trace=trace)
    else:
        b = e.batch(prm, [g["in_t_cam_obj_init"]], [g["in_pts"]], [g["in_rays"]], [g["in_depth"]], [g["in_code"]] if "in_code" in g.files else None, trace=trace)
    return b, cfg, oprm, dec, cfg["optimizer"]["code_len"], g["it_H"].shape[0]


def _record(engines, name, weights="mean"):
    """The level-2 record of the golden's run (its own iteration count), computed once per (golden, weights)."""
    if (name, weights) not in _RECORDS:
        b, cfg, _, _, code_len, n_it = _golden_batch(engines, name)
        b.set_posterior(2, weights)
        b.run()
        rows, rec = b.results(), b.posterior()
        b.close()
        assert rows[3][0] == 0 and rec["status"][0] == OK
        _RECORDS[(name, weights)] = (rec, rows, cfg, code_len)
    return _RECORDS[(name, weights)]


@pytest.mark.parametrize("name", CHAIN)
def test_record_is_the_iterations_own_linearisation(engines, name):
    rec, rows, cfg, code_len = _record(engines, name)
    pose_only = cfg is None
    b2, _, _, _, _, _ = _golden_batch(engines, name, trace=True)
    if pose_only:
        b2.set_start_state([rec["t_obj_cam"][0]])
    else:
        b2.set_start_state([rec["t_obj_cam"][0]], [rec["code"][0]])          # depths: derived on the device from the pose
    b2.set_iterations(1)
    b2.run()
    tr, (_, _, loss2, status2) = b2.trace(0), b2.results()
    b2.close()
    assert status2[0] == 0
    assert np.array_equal(tr["t_obj_cam"][0], rec["t_obj_cam"][0])
    n = 6 if pose_only else 71
    s_damp = 0.0 if pose_only else cfg["optimizer"]["joint_optim"]["scale_damping"]
    h = R.with_damping(rec["Lambda"][0][:n, :n], s_damp, code_len, pose_only).astype(np.float32)
    g32 = rec["g"][0][:n].astype(np.float32)
    print(name, "M V K", rec["M"][0], rec["V"][0], rec["K"][0], "trace V K", tr["V"][0], tr["K"][0], "loss", rec["loss"][0], loss2[0],
          "H entries differing", int((h != tr["H"][0]).sum()), "b entries differing", int((g32 != tr["b"][0]).sum()))
    assert np.array_equal(h, tr["H"][0])
    assert np.array_equal(g32, tr["b"][0])
    if pose_only:
        assert int(tr["K"][0]) == int(rec["M"][0]) == 300            # the trace's K of a pose-only batch: the points of the system
    else:
        assert int(tr["V"][0]) == int(rec["V"][0]) and int(tr["K"][0]) == int(rec["K"][0])
        assert np.array_equal(tr["code"][0][:code_len], rec["code"][0]) and np.array_equal(tr["depths"][0], rec["depths"][0])
        assert rec["loss"][0] == loss2[0]
        assert not rec["Lambda"][0][7 + code_len:].any() and not rec["Lambda"][0][:, 7 + code_len:].any() and not rec["var_code"][0][code_len:].any()
    # the state is the one the first run returned: t_cam_obj is its inverse
    t_co = np.linalg.inv(rec["t_obj_cam"][0].astype(np.float64))
    if pose_only:
        t_co[:3, :3] /= float(golden(name)["scale"])
    assert np.abs(t_co - rows[0][0]).max() <= 1e-5 * np.abs(rows[0][0]).max()


def test_filtered_pose_only_set(eng, oracle_decoder):
    """Eight iterations with planted outliers: the record is built from the points alive at the end of the run."""
    g = golden("golden_pose_only_8it.npz")
    b = _pose_batch(eng, _pose_objects()[:1], 8)
    b.set_posterior(2, "mean")
    b.run()
    rec = b.posterior()
    b.close()
    assert rec["status"][0] == OK and int(rec["M"][0]) == int(g["it_n"][-1]) < 300
    ref = O.pose_only_system(oracle_decoder, g["pts"][g["mask_e4"]], rec["t_obj_cam"][0], g["code"])
    assert ref["n"] == int(g["it_n"][-1])
    h_ref = ref["H"].astype(np.float64) - 1e-2 * np.eye(6)
    err = np.abs(rec["Lambda"][0][:6, :6] - h_ref).max() / np.abs(ref["H"]).max()
    print("filtered pose-only set: M %d, |Lambda - (H_oracle - 1e-2 I)| / max|H| = %.2e" % (rec["M"][0], err))
    assert err <= 1e-4


def test_sum_weights_pose_only(eng):
    recs = {}
    for w in ("mean", "sum"):
        b = _pose_batch(eng, _pose_objects()[:2], 8)
        b.set_posterior(2, w)
        b.run()
        recs[w] = b.posterior()
        b.close()
    for i in range(2):
        m = float(recs["mean"]["M"][i])
        a, s = recs["mean"]["Lambda"][i][:6, :6] * m, recs["sum"]["Lambda"][i][:6, :6]
        assert np.all(np.abs(a - s) <= 4 * np.spacing(np.abs(s)))
        assert recs["sum"]["M"][i] == recs["mean"]["M"][i] and recs["sum"]["status"][i] == OK


def test_sum_weights_joint_against_fp64(engines):
    """golden_recon_small at level 2 with SUM weights: Lambda against N Ds + K Dr + the priors of the fp64 linearisation at the record's state
    on the oracle's own fp32 sets, entry by entry in gn_metric's metric (its scales times the same factors, its allowances, TAU_H as it stands;
    the ReLU-kink allowance, given as one matrix for both terms, is scaled by the larger of the two factors)."""
    name = "golden_recon_small.npz"
    g = golden(name)
    rec, _, cfg, code_len = _record(engines, name, "sum")
    mean, _, _, _ = _record(engines, name, "mean")
    _, dec = engines(64)
    oprm = O.GNParams.from_configs(cfg)
    t, z, d = rec["t_obj_cam"][0], rec["code"][0], rec["depths"][0][:oprm.num_depth_samples]
    assert np.array_equal(t, mean["t_obj_cam"][0]) and rec["loss"][0] == mean["loss"][0]                    # the weights change no state and no loss
    ot = F.oracle_linearisation(dec, oprm, g["in_pts"], g["in_rays"], g["in_depth"], t, z, d)
    assert (int(ot["V"]), int(ot["K"])) == (int(rec["V"][0]), int(rec["K"][0])), "the oracle's sets differ at this state: pick another iteration count"
    lin = O.linearise_fp64(dec, oprm, g["in_pts"], g["in_rays"], g["in_depth"], t, z, d, ot["sets"])
    n_s, n_k = lin["N"], lin["K"]
    assert n_s == int(rec["M"][0])
    ref = n_s * lin["Ds"] + n_k * lin["Dr"] + lin["H_code_prior"] + lin["H_rot"]
    dsum = np.diag(n_s * lin["Ds"] + n_k * lin["Dr"])
    sh = np.sqrt(np.outer(dsum, dsum))
    allow = 4 * M.ulp32(ref) + M._rot_allowances(lin, oprm.k4)[0] + max(n_s, n_k) * lin["H_flip"]
    scaled = np.maximum(np.abs(rec["Lambda"][0] - ref) - allow, 0) / np.maximum(sh, 1e-300)
    print("SUM weights against fp64: worst scaled error %.2e (TAU_H %.1e), N %d K %d" % (scaled.max(), M.TAU_H, n_s, n_k))
    assert scaled.max() <= M.TAU_H
    # information grows with the observations: the SUM data part is the MEAN data part re-weighted
    assert np.trace(rec["info_pose"][0]) > np.trace(mean["info_pose"][0])


@pytest.mark.parametrize("name", CHAIN)
def test_the_inverse(engines, name):
    """cov_pose, var_code and info_pose against numpy.linalg.inv refined by two Newton-Schulz steps in long double: the device's max-norm error
    (relative to the output's largest entry) is at most max(8 e_lapack, 1e-13), e_lapack = the same error of plain float64 numpy.linalg.inv."""
    rec, _, cfg, code_len = _record(engines, name)
    pose_only = cfg is None
    n_pose = 6 if pose_only else 7
    n = 6 if pose_only else 7 + code_len
    lam = rec["Lambda"][0][:n, :n]
    assert _sym(lam) and _sym(rec["info_pose"][0]) and _sym(rec["cov_pose"][0])
    ref = R.marginals(R.refined_inverse(lam), n_pose)
    lap = R.marginals(np.linalg.inv(lam), n_pose)
    got = (rec["cov_pose"][0], rec["var_code"][0][:n - n_pose], rec["info_pose"][0])
    bound = 0.0
    for key, dv, r, l in zip(("cov_pose", "var_code", "info_pose"), got, ref, lap):
        if r.size == 0:
            continue
        e_dev, e_lap = R.rel_err(dv, r), R.rel_err(l, r)
        print(name, key, "device error %.2e, lapack %.2e, ratio %.2f" % (e_dev, e_lap, e_dev / max(e_lap, 1e-300)))
        assert e_dev <= max(8 * e_lap, 1e-13), key
        bound = max(bound, 8 * e_lap, 1e-13)
    prod = rec["info_pose"][0] @ rec["cov_pose"][0]
    cond = float(np.linalg.cond(rec["info_pose"][0]))
    print(name, "|info cov - I| %.2e, cond(info_pose) %.3g" % (np.abs(prod - np.eye(n_pose)).max(), cond))
    assert np.abs(prod - np.eye(n_pose)).max() <= bound * cond
    if not pose_only:
        k3 = float(np.float32(cfg["optimizer"]["joint_optim"]["k3"]))
        assert np.all(got[1] > 0) and np.all(got[1] <= 1.0 / k3)             # the prior alone bounds the code variance
    # the kernel's elimination restated in numpy (no fused multiply-add there: a few ulp of the entries, far inside the bound above)
    emu = R.sweep(lam, n_pose)
    assert emu["status"] == 0
    for key in ("cov_pose", "info_pose"):
        assert R.rel_err(rec[key][0], emu[key]) <= 1e-12, key


def test_singular(eng):
    """Three points give a 6 x 6 system of rank <= 3: flagged, not inverted; the neighbour and both results are untouched."""
    objs = _pose_objects()[:2]
    thin = (objs[1][0], objs[1][1], objs[1][2][:3], objs[1][3])
    out = {}
    for level in (0, 1):
        b = _pose_batch(eng, [thin, objs[1]], 3)
        b.set_posterior(level, "mean")
        b.run()
        out[level] = (b.results(), b.posterior() if level else None)
        b.close()
    rec = out[1][1]
    assert _same(out[0][0], out[1][0])
    assert rec["status"].tolist() == [SINGULAR, OK] and rec["M"].tolist() == [3, 200]
    assert not rec["cov_pose"][0].any() and rec["info_pose"][0].any() and _sym(rec["info_pose"][0])
    assert np.linalg.matrix_rank(rec["info_pose"][0], tol=1e-6 * np.abs(rec["info_pose"][0]).max()) <= 3
    b = _pose_batch(eng, [objs[1]], 3)
    b.set_posterior(1, "mean")
    b.run()
    alone = b.posterior()
    b.close()
    assert _same_record(alone, rec, 0, 1)


def test_independence(eng, ragged):
    prm, objs = ragged
    b = _joint_batch(eng, objs, prm)
    b.set_posterior(2, "sum")
    b.run()
    whole = b.posterior()
    b.close()
    for i, o in enumerate(objs):
        b = _joint_batch(eng, [o], prm)
        b.set_posterior(2, "sum")
        b.run()
        alone = b.posterior()
        b.close()
        assert _same_record(alone, whole, 0, i, L1_KEYS + ("Lambda", "g", "t_obj_cam", "code", "depths")), i


def test_partial_rerun_keeps_the_records(oracle_decoder, ragged):
    """A forced bf16 margin of 2e-5 trips the prepass guard (tests/test_gpu_prepass.py): the tripped objects run again with the prepass off, pass
    included, and the objects left out keep the record of the first run as they keep their row.  Both are the prepass-off run's, bit for bit."""
    prm, objs = ragged
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    out = {}
    for name, mode, delta in (("off", L.PREPASS_OFF, -1.0), ("trip", L.PREPASS_BF16, 2e-5)):
        b = _joint_batch(own, objs, prm)
        b.set_prepass(mode, delta)
        b.set_posterior(2, "sum")
        b.run()
        out[name] = (b.results(), b.posterior(), b.stats())
        b.close()
    own.close()
    st = out["trip"][2]
    print("guard trips", st["prepass_guard_trips"], "objects re-run", st["prepass_guard_objects"], "of", len(objs))
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_trips"] > 0
    assert _same(out["trip"][0], out["off"][0])
    assert _same_record(out["trip"][1], out["off"][1], slice(None), slice(None), L1_KEYS + ("Lambda", "g", "t_obj_cam", "code", "depths"))
    assert out["trip"][1]["status"].tolist() == [OK, OK, OK, NONE]


def test_refused_arguments(eng, ragged):
    prm, objs = ragged
    b = _joint_batch(eng, objs[:1], prm)
    lib = L.load()
    b.set_posterior(1, "sum")
    for bad in ((-1, 0), (3, 0), (1, 2), (1, -1)):
        assert lib.dsp_batch_posterior(b._h, *bad) == -1
    with pytest.raises(ValueError):
        b.set_posterior(1, "both")
    b.run()
    rec = b.posterior()
    assert rec["status"][0] == OK and "Lambda" not in rec
    lam = np.zeros((1, 71, 71))
    assert lib.dsp_batch_posterior_fetch(b._h, *([None] * 8), L.ptr(lam, L.c_f64p), None, None, None, None) == -4          # level 1 keeps no Lambda
    # the refused settings left "sum" in force: the record is the one of a fresh batch with "sum"
    b2 = _joint_batch(eng, objs[:1], prm)
    b2.set_posterior(1, "sum")
    b2.run()
    assert _same_record(rec, b2.posterior(), 0, 0)
    # switched off again: the next run returns the same rows and hands out no record of the earlier run beside them
    rows = b.results()
    b.set_posterior(0)
    b.run()
    assert _same(rows, b.results())
    assert lib.dsp_batch_posterior_fetch(b._h, *([None] * 13)) == -4
    with pytest.raises(L.DspError):
        b.posterior()
    b.set_posterior(1, "sum")
    b.run()
    assert _same(rows, b.results()) and _same_record(rec, b.posterior(), 0, 0)
    b.close()
    b2.close()


def test_through_the_top(tmp_path, eng, ragged):
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    sys.path.insert(0, pkg)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
            del sys.modules[m]
        from reconstruct.utils import get_configs, get_decoder
        from reconstruct.optimizer import Optimizer
        import reoptimise_map as RM
        cfg_d = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
        cfg_d.update(data_type="KITTI", DeepSDF_DIR=fixtures.materialize_decoder_dir("cars", str(tmp_path / "cars_64")))
        with open(tmp_path / "off.json", "w") as f:
            json.dump(cfg_d, f)
        cfg_d["optimizer"]["joint_optim"]["posterior"] = "sum"
        cfg_d["optimizer"]["pose_only_optim"]["posterior"] = "sum"
        with open(tmp_path / "on.json", "w") as f:
            json.dump(cfg_d, f)
        cfg_off, cfg_on = get_configs(str(tmp_path / "off.json")), get_configs(str(tmp_path / "on.json"))
        dec = get_decoder(cfg_on)
        off, on = Optimizer(dec, cfg_off), Optimizer(dec, cfg_on)
        off.verbose = on.verbose = False
        # (tests/golden/golden_dropin.npz holds what the drop-in loaders read -- calibration rows, two LiDAR points, import names -- and no
        # optimiser input: no surface points, rays or depths.  The detection is therefore a synthetic one, through the golden KITTI config.)
        o = synth.make_object(410, n_surface=200, n_background=50)
        r0 = off.reconstruct_object(o["t_cam_obj_init"], o["pts"], o["rays"], o["depth"])
        r1 = on.reconstruct_object(o["t_cam_obj_init"], o["pts"], o["rays"], o["depth"])
        assert r0.is_good and r1.is_good and np.array_equal(r0.t_cam_obj, r1.t_cam_obj) and np.array_equal(r0.code, r1.code) and float(r0.loss) == float(r1.loss)
        with pytest.raises(KeyError):
            r0.pose_information
        with pytest.raises(KeyError):
            r0["posterior_ok"]
        b = dec.engine.batch(on._params(), [o["t_cam_obj_init"]], [o["pts"]], [o["rays"]], [o["depth"]])
        b.set_posterior(1, "sum")
        b.run()
        rec = b.posterior()
        b.close()
        assert r1.posterior_ok is True and np.array_equal(r1.pose_information, rec["info_pose"][0]) and np.array_equal(r1.pose_covariance, rec["cov_pose"][0])
        assert np.array_equal(r1.code_variance, rec["var_code"][0]) and r1.loss_at_result == float(rec["loss"][0])
        scale = np.cbrt(np.linalg.det(r1.t_cam_obj[:3, :3].astype(np.float64)))
        omega = P.edge_information(r1.pose_information, scale)
        assert np.array_equal(omega, omega.T) and np.all(np.linalg.eigvalsh(omega) > 0)
        print("edge information from the optimiser: eigenvalues", np.linalg.eigvalsh(omega), "(the constant it replaces: 1e3)")
        # pose-only: the tensor alone from the reference's method; the batched form on request with the record
        g = golden("golden_pose_only.npz")
        t_ref = off.estimate_pose_cam_obj(g["t_co_se3"], float(g["scale"]), g["pts"], g["code"])
        poses, post = on.estimate_poses_cam_obj([g["t_co_se3"]], [float(g["scale"])], [g["pts"]], [g["code"]], return_posterior=True)
        assert np.array_equal(t_ref.numpy(), poses[0]) and post["status"][0] == OK and post["info_pose"].shape == (1, 6, 6)
        assert np.all(np.linalg.eigvalsh(P.edge_information(post["info_pose"][0], float(g["scale"]))) > 0)
        # the map tool: one record per map object, whatever it observed; poses and codes as without the flag
        gm = golden("golden_map_objects.npz")
        map_dir = tmp_path / "map"
        (map_dir / "observations").mkdir(parents=True)
        objs = []
        for k, oid in enumerate(gm["ids"]):
            so = synth.make_object(420 + k, n_surface=120 + 20 * k, n_background=40)
            t_wc = np.eye(4)
            t_wc[:3, 3] = (2.0 * k, 0.0, -1.0 * k)
            objs.append(dict(id=int(oid), pose=t_wc @ so["t_cam_obj_init"].astype(np.float64), code=np.zeros(64, np.float32)))
            if k != 2:
                np.savez(map_dir / "observations" / ("%d.npz" % int(oid)), pts=so["pts"], rays=so["rays"], depth=so["depth"], t_world_cam=t_wc)
        write_map_objects(str(map_dir / "MapObjects.txt"), objs)
        import runpy
        old = sys.argv
        outs = {}
        try:
            for flag in (False, True):
                dst = str(map_dir / ("reopt%d.txt" % flag))
                sys.argv = ["reoptimise_map.py", "--config", str(tmp_path / "off.json"), "--map_dir", str(map_dir), "--gpus", "1", "--out", dst] + (
                    ["--posterior", str(tmp_path / "post.npz")] if flag else [])
                runpy.run_path(os.path.join(ROOT, "tools", "reoptimise_map.py"), run_name="__main__")
                outs[flag] = open(dst).read()
        finally:
            sys.argv = old
        assert outs[False] == outs[True]
        z = np.load(str(tmp_path / "post.npz"))
        assert z["ids"].tolist() == [int(i) for i in gm["ids"]] and z["status"].tolist() == [OK, OK, NONE, OK]
        assert z["info_pose"].shape == (4, 7, 7) and z["info_pose"][0].any() and not z["info_pose"][2].any()
        dec.engine.close()
    finally:
        sys.path.remove(pkg)
        sys.path.remove(os.path.join(ROOT, "tools"))
        for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
            del sys.modules[m]


def test_low_precision_compute_mode(eng):
    """One object in the f16 compute mode, forced onto a detection-sized batch: the pass runs in that mode; a valid record, and its distance from
    the fp32 record is reported."""
    o = synth.make_object(402, n_surface=250, n_background=200)
    prm = E.gn_params(num_iterations=4)
    recs, rows = {}, {}
    for mode in ("f32", "f16", "f16_off"):
        b = _joint_batch(eng, [o], prm)
        if mode != "f32":
            b.set_compute(L.COMPUTE_F16)
            b.set_lp_small_batches(1)
        b.set_posterior(0 if mode == "f16_off" else 1, "mean")
        b.run()
        rows[mode] = b.results()
        recs[mode] = b.posterior() if mode != "f16_off" else None
        b.close()
    assert _same(rows["f16"], rows["f16_off"]) and not _same(rows["f16"], rows["f32"])
    r = recs["f16"]
    assert r["status"][0] == OK and _sym(r["info_pose"]) and _sym(r["cov_pose"])
    assert np.all(np.linalg.eigvalsh(r["info_pose"][0]) > 0) and np.all(np.linalg.eigvalsh(r["cov_pose"][0]) > 0) and np.all(r["var_code"][0] > 0)
    print("f16 compute mode: relative difference of info_pose to the fp32 record %.2e, of cov_pose %.2e" % (
        F.rel_max(r["info_pose"][0], recs["f32"]["info_pose"][0]), F.rel_max(r["cov_pose"][0], recs["f32"]["cov_pose"][0])))
