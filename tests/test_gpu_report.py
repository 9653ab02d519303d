"""GPU: the observation report (dsp_batch_report / dsp_batch_report_fetch, include/dsp_gn.h) -- every surface point and every ray evaluated
once more at the state the run returns.

  * neutrality: result rows, iterations used, traces, the step log, level-2 posterior records and the prior's residual are bit-equal with
    the report on and off, for joint, multi-view and pose-only batches; a batch that had the report switched on and off again launches what
    a batch that never had it launches;
  * device against host arithmetic: dsp_debug_report_ray (csrc/report_math.h on the CPU) on the sdf grid the pass left
    (Batch.debug_samples) and the record's depths reproduces depth, hit, residual and the three counts of EVERY ray bit for bit, at
    num_depth_samples 50 and 64 (range_mask was wrong at 64 until cc6816d) and, at a pinned state with kept rows, 2;
  * device against the oracle, at the level-2 record's t_obj_cam, code and depths: pt_sdf and the three ray floats within
    4 x TAU + 4 ulp32 of the fp64 twin (tests/report_ref.py; TAU measured on the CPU by tools/measure_report.py), M, V and the in-sphere
    counts equal, band and kept counts equal on every ray whose threshold decisions agree between the fp32 oracle, its sdf_jitter twins and
    fp64 (at most 0.5 % of a case's rays may be left out), the sums within their bounds, and k2 sum_s / M + k1 sum_r / K against the
    posterior's loss.  The band count is informational where early ray termination or the prepass skip samples behind a solid one (dsp_gn.h),
    so this comparison runs with every in-sphere sample decoded (set_ray_passes(1), prepass off: settings that change no result bit), and
    the default settings are held to the same floats and kept counts bit for bit;
  * the pose-only alive bits are the mask oracle.estimate_pose_cam_obj ends with, M the alive count;
  * failed members: NaN rows, zero counts, the status word; a view without rays keeps its points;
  * with the convergence rule, step control, the f16 compute mode, forced guard trips (every good object re-run; one re-run while another
    good member is left out and keeps its first-run rows), and an injected allocation failure at enable.

Every comparison prints its figure before it asserts; the figures of an MI355X run are in profiles/report.md.
"""
import numpy as np
import pytest

import multiview_oracle as MV
import report_ref as R
from conftest import golden
from oracle import dsp_oracle as O
from dsp_slam_amd import _lib as L, engine as E

pytestmark = pytest.mark.gpu
F32 = np.float32
N_IT = R.N_IT
REPORT_KEYS = ("pt_sdf", "pt_flags", "ray_depth", "ray_hit", "ray_residual", "ray_counts", "M", "V", "m", "K", "sum_s", "sum_r", "status")
POST_KEYS = ("status", "info_pose", "cov_pose", "var_code", "loss", "M", "V", "K", "Lambda", "g", "t_obj_cam", "code", "depths")


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def objs():
    return R.joint_objects()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _joint(eng, objs, prm, trace=False):
    return eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                     [np.zeros(64, F32) for _ in objs], trace=trace)


def _everything(b, n_it, views=False, posterior=True, prior=False, steps=False):
    """All a run returns besides the report."""
    b.run()
    out = list(b.results()) + [b.iterations_used()]
    for e in range(n_it):
        tr = b.trace(e)
        out += [tr[k] for k in sorted(tr)]
        if views:
            tv = b.trace_views(e)
            out += [tv[k] for k in sorted(tv)]
    if posterior:
        rec = b.posterior()
        out += [rec[k] for k in POST_KEYS]
    if prior:
        pr = b.prior_residual()
        out += [pr["e"], pr["chi2"]]
    if steps:
        sl = b.step_log()
        out += [sl[k] for k in sorted(sl)]
    return out


def _report_rows(rep):
    return [rep[k] for k in REPORT_KEYS]


def _cut(rep, key, i):
    off = rep["pts_off"] if key.startswith("pt_") else rep["ray_off"]
    return rep[key][off[i]:off[i + 1]]


def _host_rays(rep, i, sdf_grid, depths, depth_fg, th):
    """dsp_debug_report_ray on every ray of member i -> (floats (n_rays, 3), counts (n_rays, 3))."""
    lib = L.load()
    n_rays, n_d = sdf_grid.shape
    d = L.f32(depths[:n_d])
    fl, cn = np.zeros((n_rays, 3), F32), np.zeros((n_rays, 3), np.int32)
    out4, c3 = np.zeros(4, F32), np.zeros(3, np.int32)
    for r in range(n_rays):
        row = L.f32(sdf_grid[r])
        fg = r < depth_fg.shape[0]
        assert lib.dsp_debug_report_ray(n_d, L.ptr(d), L.ptr(row), float(th), float(depth_fg[r]) if fg else 0.0, int(fg), L.ptr(out4), L.ptr(c3, L.c_i32p)) == 0
        fl[r], cn[r] = out4[:3], c3
    return fl, cn


def _check_against_host(b, rep, rec, members, inputs, n_depth, th, ray_w=None):
    """Every evaluated member: the device's rays are the host function's, bit for bit.  ray_w (per member, optional): the observation
    weights -- a ray of weight 0 is absent, its rows those of a member without a render term (NaN floats, zero counts)."""
    n = 0
    for i in members:
        rays, depth = inputs[i]
        if rays.shape[0] == 0:
            continue
        _, sdf, _ = b.debug_samples(i, rays.shape[0], n_depth)
        fl, cn = _host_rays(rep, i, sdf, rec["depths"][i], depth, th)
        if ray_w is not None:
            fl[np.asarray(ray_w[i]) == 0], cn[np.asarray(ray_w[i]) == 0] = np.nan, 0
        for k, key in enumerate(("ray_depth", "ray_hit", "ray_residual")):
            assert _bits(_cut(rep, key, i), fl[:, k]), (i, key, np.abs(_cut(rep, key, i) - fl[:, k]).max())
        assert np.array_equal(_cut(rep, "ray_counts", i), cn), i
        n += rays.shape[0]
    return n


# ---- neutrality, and the device against the host arithmetic ------------------------------------------------------------------------------
@pytest.mark.parametrize("n_depth", [50, 64])
def test_joint_neutral_and_bit_equal_to_the_host_arithmetic(eng, objs, n_depth):
    prm = E.gn_params(num_iterations=N_IT, num_depth_samples=n_depth)
    got, reps = {}, {}
    for mode in ("off", "on", "on_alone", "off_again"):
        b = _joint(eng, objs, prm, trace=True)
        post = mode != "on_alone"
        if post:
            b.set_posterior(2, "mean")
        if mode != "off":
            b.set_report(True)
        if mode == "off_again":
            b.set_report(False)
        got[mode] = _everything(b, N_IT, posterior=post)
        st = b.stats()
        got[mode + "_launches"] = (st["n_mlp_fwd_launches"], st["n_mlp_jac_launches"], st["n_mlp_prepass_launches"])
        if mode in ("on", "on_alone"):
            reps[mode] = b.report()
            if mode == "on":
                rec = b.posterior()
                n = _check_against_host(b, reps[mode], rec, [0, 1], [(o["rays"], o["depth"]) for o in objs], n_depth, prm.cut_off)
                assert n == objs[0]["rays"].shape[0] + objs[1]["rays"].shape[0]
        else:
            assert L.load().dsp_batch_report_fetch(b._h, *([None] * 7)) == -4               # DSP_E_STATE: the last run had no report
        b.close()
    assert got["off"][3].tolist() == [0, 0, L.OBJ_FEW_SAMPLES]
    assert _same(got["off"], got["on"]) and _same(got["off"], got["off_again"])
    assert _same(got["off"][:len(got["on_alone"])], got["on_alone"])                        # results, iterations, traces: the report alone changes none
    assert got["off_launches"] == got["off_again_launches"] == got["on_launches"]            # the posterior's pass is shared; off again = never on
    assert got["on_alone_launches"] == got["on_launches"]                                    # ... and the report alone runs that same front
    assert _same(_report_rows(reps["on"]), _report_rows(reps["on_alone"]))                  # the same rows with and without the posterior beside it
    # a batch without the posterior and without the report launches less: the pass is not there
    b = _joint(eng, objs, prm)
    b.run()
    st = b.stats()
    assert st["n_mlp_jac_launches"] < got["on_launches"][1]
    b.close()
    # the failed member: NaN rows, zero counts and flags, its status word
    rep = reps["on"]
    assert rep["status"].tolist() == [0, 0, L.OBJ_FEW_SAMPLES] and rep["M"][2] == 0 and rep["K"][2] == 0
    for key in ("pt_sdf", "ray_depth", "ray_hit", "ray_residual"):
        assert np.isnan(_cut(rep, key, 2)).all() and not np.isnan(_cut(rep, key, 0)).any() and not np.isnan(_cut(rep, key, 1)).any(), key
    assert not _cut(rep, "ray_counts", 2).any() and not _cut(rep, "pt_flags", 2).any() and np.isnan(rep["sum_s"][2]) and np.isnan(rep["sum_r"][2])
    assert _cut(rep, "pt_flags", 0).all() and _cut(rep, "pt_flags", 1).all()
    assert rep["pts_off"].tolist() == [0, 120, 217, 281] and rep["ray_off"].tolist() == [0, 100, 205, 289] and rep["view_off"].tolist() == [0, 1, 2, 3]


def test_two_depth_samples(eng, oracle_decoder, objs):
    """num_depth_samples = 2, the smallest the library takes.  The two samples an iteration derives from the pose sit on the unit sphere's
    rim (t_z -+ scale), where no ray has an in-sphere sample, so the state is pinned instead: the ground-truth pose and code, a learning
    rate of 0, and a depth schedule whose row behind the run's one iteration is what the pass samples -- a depth on the visible surface
    and one half a metre behind it.  The fp32 oracle says on the CPU that both objects have kept rows there; the device's rows are the
    host arithmetic's bit for bit and its counts are the oracle's."""
    two = objs[:2]
    prm = E.gn_params(num_iterations=1, num_depth_samples=2, lr=0.0)
    oprm = R.oracle_params(2)
    t_oc = [O._inv(o["t_cam_obj_gt"]) for o in two]
    depths = [np.array([np.median(o["depth"]), np.median(o["depth"]) + 0.5], F32) for o in two]
    b = _joint(eng, two, prm)
    b.set_start_state(t_oc, [o["code_gt"] for o in two])
    b.set_depth_schedule([depths, depths])
    b.set_ray_passes(1)
    b.set_prepass(L.PREPASS_OFF)
    b.set_posterior(2, "mean")
    b.set_report(True)
    b.run()
    rep, rec = b.report(), b.posterior()
    print("D = 2: status", rep["status"], "V", rep["V"], "m", rep["m"], "K", rep["K"])
    assert rep["status"].tolist() == [0, 0] and (rep["K"] > 0).all() and (rep["V"] >= 10).all()
    assert all(np.array_equal(rec["depths"][i][:2], depths[i]) for i in range(2))
    assert _check_against_host(b, rep, rec, [0, 1], [(o["rays"], o["depth"]) for o in two], 2, prm.cut_off) == 205
    b.close()
    for i, o in enumerate(two):
        r32 = R.evaluate32(oracle_decoder, oprm, o["pts"], o["rays"], o["depth"], rec["t_obj_cam"][i], rec["code"][i], depths[i])
        ok = R.agreeing_rays(oracle_decoder, oprm, o["pts"], o["rays"], o["depth"], rec["t_obj_cam"][i], rec["code"][i], depths[i], r32)
        assert r32["K"] > 0 and rep["V"][i] == r32["V"] and np.array_equal(_cut(rep, "ray_counts", i)[ok], r32["ray_counts"][ok]) and ok.any()


# ---- the device against the oracle ---------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return float(np.spacing(np.abs(F32(x))))


def _check_member_against_oracle(dec, oprm, prm, rep, i, pts, rays, depth, t_oc, code, depths, what):
    r32 = R.evaluate32(dec, oprm, pts, rays, depth, t_oc, code, depths)
    r64 = R.evaluate64(dec, oprm, pts, rays, depth, t_oc, code, depths, r32["in_mask"])
    fig = {}
    for key in ("pt_sdf", "ray_depth", "ray_hit", "ray_residual"):
        got = _cut(rep, key, i).astype(np.float64)
        err = np.abs(got - r64[key])
        fig[key] = float(err.max()) if err.size else 0.0
        print("%s member %d %s: worst |device - fp64| %.3g (4 TAU = %.3g)" % (what, i, key, fig[key], 4 * R.TAU[key]))
        assert (err <= R.bound(key, r64[key])).all(), (what, i, key, fig[key])
    assert rep["M"][i] == r32["M"] and rep["V"][i] == r32["V"]
    cn = _cut(rep, "ray_counts", i)
    assert np.array_equal(cn[:, 0], r32["ray_counts"][:, 0])
    ok = R.agreeing_rays(dec, oprm, pts, rays, depth, t_oc, code, depths, r32, r64)
    assert np.array_equal(cn[ok], r32["ray_counts"][ok]), (what, i)
    # sum_r is a sum over the kept rows, each carrying its ray's residual: the reference is the fp64 sum over the fp32 oracle's kept set, for
    # EVERY member.  On a ray left out of the count comparison the device may keep other rows than the fp32 oracle: each such row moves the
    # sum by at most rho(0.30) = 0.08 (report_ref.HUBER_ROW_MAX), and only those rows widen the bound.
    differing = int(np.abs(cn[~ok, 2] - r32["ray_counts"][~ok, 2]).sum())
    for key, ref, extra in (("sum_s", r64["sum_s"], 0.0), ("sum_r", R.sum_r64_on(r64, r32["ray_counts"][:, 2], oprm.b1), R.HUBER_ROW_MAX * differing)):
        err = abs(rep[key][i] - ref)
        print("%s member %d %s: device %.9g fp64 %.9g |diff| %.3g (4 TAU = %.3g, rows kept differently %d)" % (
            what, i, key, rep[key][i], ref, err, 4 * R.TAU[key], differing if key == "sum_r" else 0))
        assert err <= R.bound(key, ref) + extra, (what, i, key, err)
    return int(ok.shape[0]), int((~ok).sum()), r32, ok


@pytest.mark.parametrize("n_depth", [50, 64])
def test_device_matches_the_oracle(eng, oracle_decoder, objs, n_depth):
    """At the level-2 record's state, with every in-sphere sample decoded; the default settings give the same floats and kept counts.  The loss
    formed from the sums is held to the posterior's float32 loss to 4 ulp32."""
    prm = E.gn_params(num_iterations=N_IT, num_depth_samples=n_depth)
    oprm = R.oracle_params(n_depth)
    reps = {}
    for mode in ("every_sample", "default"):
        b = _joint(eng, objs, prm)
        if mode == "every_sample":
            b.set_ray_passes(1)
            b.set_prepass(L.PREPASS_OFF)
        b.set_posterior(2, "mean")
        b.set_report(True)
        b.run()
        reps[mode] = (b.report(), b.posterior(), b.results())
        b.close()
    rep, rec, res = reps["every_sample"]
    dflt = reps["default"][0]
    # the default settings: the same floats and kept / in-sphere counts, bit for bit; the band count may miss samples behind a solid one
    assert _same(res, reps["default"][2])
    for key in REPORT_KEYS:
        if key not in ("ray_counts", "m"):
            assert _bits(rep[key], dflt[key]), key
    assert np.array_equal(rep["ray_counts"][:, [0, 2]], dflt["ray_counts"][:, [0, 2]]) and (dflt["ray_counts"][:, 1] <= rep["ray_counts"][:, 1]).all()
    n_rays = n_out = 0
    for i in (0, 1):
        o = objs[i]
        a, c, r32, ok = _check_member_against_oracle(oracle_decoder, oprm, prm, rep, i, o["pts"], o["rays"], o["depth"], rec["t_obj_cam"][i], rec["code"][i],
                                                     rec["depths"][i][:n_depth], "joint D=%d" % n_depth)
        n_rays, n_out = n_rays + a, n_out + c
        # the default settings' band count: every band sample up to a ray's first solid sample is decoded and counted; those behind it
        # (T = 0 there) may or may not be -- so it lies between the oracle's count up to the first solid sample and the oracle's full count
        lo, hi, got = R.band_up_to_first_solid(r32, prm.cut_off)[ok], r32["ray_counts"][ok, 1], _cut(dflt, "ray_counts", i)[ok, 1]
        print("joint D=%d member %d: band samples at default settings %d, oracle up to the first solid sample %d, oracle all %d" % (
            n_depth, i, got.sum(), lo.sum(), hi.sum()))
        assert (lo <= got).all() and (got <= hi).all()
        assert rep["M"][i] == rec["M"][i] and rep["V"][i] == rec["V"][i] and rep["K"][i] == rec["K"][i]
        assert rep["K"][i] == _cut(rep, "ray_counts", i)[:, 2].sum() and rep["m"][i] == _cut(rep, "ray_counts", i)[:, 1].sum()
        # a single-view object's k2 sum_s / M + k1 sum_r / K is the loss at the returned state (k_posterior's float32 arithmetic)
        loss = F32(prm.k1) * (F32(rep["sum_r"][i]) / F32(rep["K"][i])) + F32(prm.k2) * (F32(rep["sum_s"][i]) / F32(rep["M"][i]))
        print("joint D=%d member %d: loss from the sums %.9g, posterior %.9g, %.2f ulp32" % (
            n_depth, i, loss, rec["loss"][i], abs(float(loss) - float(rec["loss"][i])) / _ulp32(rec["loss"][i])))
        assert abs(float(loss) - float(rec["loss"][i])) <= 4 * _ulp32(rec["loss"][i])
    print("joint D=%d: %d of %d rays left out of the count comparison" % (n_depth, n_out, n_rays))
    assert n_out <= 0.005 * n_rays


# ---- multi-view -------------------------------------------------------------------------------------------------------------------------------
def test_multiview(eng, oracle_decoder):
    mv = R.multiview_objects()
    prm = E.gn_params(num_iterations=N_IT)
    oprm = R.oracle_params(50)
    got, rep, rec = {}, None, None
    for mode in ("off", "on"):
        b = eng.multiview_batch(prm, [o["t_cam_obj_init"] for o in mv], [o["views"] for o in mv], [np.zeros(64, F32)] * 2, trace=True)
        b.set_posterior(2, "mean")
        if mode == "on":
            b.set_report(True)
        got[mode] = _everything(b, N_IT, views=True)
        if mode == "on":
            rep, rec = b.report(), b.posterior()
        b.close()
    assert _same(got["off"], got["on"]) and got["off"][3].tolist() == [0, 0]
    views = [v for o in mv for v in o["views"]]
    assert rep["view_off"].tolist() == [0, 3, 4] and rep["pts_off"].tolist() == [0, 90, 180, 270, 380] and rep["ray_off"].tolist() == [0, 120, 120, 240, 380]
    # the view without rays: no render term (DSP_OBJ_FEW_SAMPLES), but its surface points are in the pooled system and are reported
    assert rep["status"].tolist() == [0, L.OBJ_FEW_SAMPLES, 0, 0] and rep["V"][1] == 0 and rep["K"][1] == 0 and rep["sum_r"][1] == 0.0
    assert rep["M"].tolist() == [90, 90, 90, 110] and not np.isnan(rep["pt_sdf"]).any() and rep["pt_flags"].all() and (rep["sum_s"] > 0).all()
    # the pooled loss from the members' sums against the posterior's
    for obj in range(2):
        m0, m1 = rep["view_off"][obj], rep["view_off"][obj + 1]
        M, K = rep["M"][m0:m1].sum(), rep["K"][m0:m1].sum()
        assert M == rec["M"][obj] and K == rec["K"][obj] and rep["V"][m0:m1].sum() == rec["V"][obj]
        loss = F32(prm.k1) * (F32(rep["sum_r"][m0:m1].sum()) / F32(K)) + F32(prm.k2) * (F32(rep["sum_s"][m0:m1].sum()) / F32(M))
        print("multi-view object %d: loss from the sums %.9g, posterior %.9g, %.2f ulp32" % (
            obj, loss, rec["loss"][obj], abs(float(loss) - float(rec["loss"][obj])) / _ulp32(rec["loss"][obj])))
        assert abs(float(loss) - float(rec["loss"][obj])) <= 4 * _ulp32(rec["loss"][obj])
    # the reference views (T_oc_v = T_oc, the record's depths) against the oracle, like a joint object
    n_rays = n_out = 0
    for obj, member in ((0, 0), (1, 3)):
        v = views[member]
        a, c, _, _ = _check_member_against_oracle(oracle_decoder, oprm, prm, rep, member, v["pts"], v["rays"], v["depth"], rec["t_obj_cam"][obj], rec["code"][obj],
                                            rec["depths"][obj][:50], "multi-view")
        n_rays, n_out = n_rays + a, n_out + c
    # the other view with rays: evaluated at T_oc_v -- pt_sdf against the fp64 decoder at the oracle's T_oc T_ref_v
    t_v, _ = MV.view_state(rec["t_obj_cam"][0], views[2]["t_ref_cam"], 50)
    t64 = np.asarray(t_v, np.float64)
    ref = O._decode64(oracle_decoder, np.asarray(rec["code"][0], np.float64), views[2]["pts"].astype(np.float64) @ t64[:3, :3].T + t64[:3, 3], grad=False)[0]
    assert (np.abs(_cut(rep, "pt_sdf", 2) - ref) <= R.bound("pt_sdf", ref)).all()
    assert n_out <= 0.005 * n_rays


# ---- pose-only -------------------------------------------------------------------------------------------------------------------------------
def test_pose_only_alive_mask(eng, oracle_decoder):
    g, g5 = golden("golden_pose_only_8it.npz"), golden("golden_pose_only.npz")
    po = [(g["t_co_se3"], float(g["scale"]), g["pts"], g["code"]), (g5["t_co_se3"], float(g5["scale"]), g5["pts"][:200], g5["code"])]
    prm = E.gn_params(pose_only_iterations=8)
    got = {}
    for mode in ("off", "on"):
        b = eng.pose_batch(prm, [o[0] for o in po], [o[1] for o in po], [o[2] for o in po], [o[3] for o in po], trace=True)
        b.set_posterior(2, "mean")
        if mode == "on":
            b.set_report(True)
        got[mode] = _everything(b, 8)
        if mode == "on":
            rep, rec = b.report(), b.posterior()
        b.close()
    assert _same(got["off"], got["on"])
    assert rep["ray_depth"].shape == (0,) and rep["ray_counts"].shape == (0, 3) and rep["pts_off"].tolist() == [0, 300, 500]
    dropped = []
    for i, o in enumerate(po):
        tr = []
        O.estimate_pose_cam_obj(oracle_decoder, O.GNParams(num_iterations_pose_only=8), o[0], o[1], o[2], o[3], trace=tr)
        mask = tr[4]["mask"]
        assert np.array_equal(_cut(rep, "pt_alive", i), mask), i
        assert rep["M"][i] == mask.sum() == rec["M"][i] and rep["status"][i] == 0 and rep["V"][i] == 0 and rep["K"][i] == 0
        dropped.append(int((~mask).sum()))
        ref = O.compute_sdf_loss(oracle_decoder, o[2], rec["t_obj_cam"][i], o[3])[2].astype(np.float64)
        sdf = _cut(rep, "pt_sdf", i)
        assert (np.abs(sdf - ref) <= R.bound("pt_sdf", ref)).all()
        # sum_s: r^2 over the alive points (the pose-only system has no robust weights)
        s = float(np.sum(sdf[mask].astype(np.float64) ** 2))
        assert abs(rep["sum_s"][i] - s) <= 1e-12 * s
    print("pose-only: points the filter dropped", dropped)
    assert dropped[0] > 0 and dropped[1] == 0            # the filter drops points in one object only


# ---- with the other optional features ---------------------------------------------------------------------------------------------------------
def _consistent_with_the_record(b, rep, rec, objs, members, prm, n_depth=50):
    """The rows belong to the state the record was taken at: host arithmetic on the record's depths, and the record's counts."""
    _check_against_host(b, rep, rec, members, [(o["rays"], o["depth"]) for o in objs], n_depth, prm.cut_off)
    for i in members:
        assert rep["M"][i] == rec["M"][i] and rep["V"][i] == rec["V"][i] and rep["K"][i] == rec["K"][i]
        loss = F32(prm.k1) * (F32(rep["sum_r"][i]) / F32(rep["K"][i])) + F32(prm.k2) * (F32(rep["sum_s"][i]) / F32(rep["M"][i]))
        assert abs(float(loss) - float(rec["loss"][i])) <= 4 * _ulp32(rec["loss"][i])


def test_with_the_convergence_rule_the_rows_are_the_frozen_state(eng, objs):
    """Object 0 warm-started from its own result freezes early; its rows are taken at the frozen state, which is the record's."""
    prm = E.gn_params(num_iterations=N_IT)
    b = _joint(eng, objs[:2], prm)
    b.run()
    t, code, _, _ = b.results()
    b.close()
    warm = [dict(objs[0], t_cam_obj_init=t[0].copy()), objs[1]]
    got = {}
    for mode in ("off", "on"):
        b = eng.batch(prm, [o["t_cam_obj_init"] for o in warm], [o["pts"] for o in warm], [o["rays"] for o in warm], [o["depth"] for o in warm],
                      [L.code64(code[0]), np.zeros(64, F32)], trace=True)
        b.set_convergence(0.5, 0.5, 2)
        b.set_posterior(2, "mean")
        if mode == "on":
            b.set_report(True)
        got[mode] = _everything(b, N_IT)
        if mode == "on":
            rep, rec = b.report(), b.posterior()
            print("convergence rule: iterations used", got[mode][4])
            assert got[mode][4].min() < N_IT
            _consistent_with_the_record(b, rep, rec, warm, [0, 1], prm)
        b.close()
    assert _same(got["off"], got["on"])


def test_with_step_control_and_a_prior_the_rows_belong_to_x_acc(eng, objs):
    prm = E.gn_params(num_iterations=8)
    two = objs[:2]
    b = _joint(eng, two, prm)
    b.set_posterior(2, "sum")
    b.run()
    first = b.posterior()
    b.close()
    lam = first["Lambda"].copy()
    lam[:, np.arange(7, 71), np.arange(7, 71)] -= float(F32(prm.k3))          # (the record contains k3 I: dsp_gn.h)
    lam = 1e-3 * 0.5 * (lam + np.swapaxes(lam, 1, 2))
    lam[:, np.arange(71), np.arange(71)] = np.abs(lam[:, np.arange(71), np.arange(71)])
    got = {}
    for mode in ("off", "on"):
        b = _joint(eng, two, prm, trace=True)
        b.set_step_control()
        b.set_prior(first["t_obj_cam"], first["code"], lam)
        b.set_posterior(2, "mean")
        if mode == "on":
            b.set_report(True)
        got[mode] = _everything(b, 8, prior=True, steps=True)
        if mode == "on":
            rep, rec = b.report(), b.posterior()
            _consistent_with_the_record(b, rep, rec, two, [0, 1], prm)
        b.close()
    assert _same(got["off"], got["on"])


def test_low_precision_mode_runs_and_keeps_its_result_bits(eng, objs):
    prm = E.gn_params(num_iterations=N_IT)
    got = {}
    for mode in ("off", "on"):
        b = _joint(eng, objs, prm)
        b.set_compute(L.COMPUTE_F16)
        b.set_lp_small_batches(1)
        if mode == "on":
            b.set_report(True)
        b.run()
        got[mode] = list(b.results()) + [b.iterations_used()]
        if mode == "on":
            rep = b.report()
            assert rep["status"].tolist() == got[mode][3].tolist() and np.isfinite(rep["ray_depth"][:205]).all() and np.isfinite(rep["pt_sdf"][:217]).all()
        b.close()
    assert _same(got["off"], got["on"])


def test_a_guard_trip_refreshes_the_rerun_objects_rows_only(oracle_decoder, objs):
    """A forced bf16 margin of 2e-5 trips the prepass guard: the tripped objects run again with the prepass off, the pass included.  Every
    object's rows -- re-run or left out -- are those of the prepass-off run, bit for bit, like its result row."""
    prm = E.gn_params(num_iterations=N_IT)
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    out = {}
    for name, mode, delta in (("off", L.PREPASS_OFF, -1.0), ("trip", L.PREPASS_BF16, 2e-5)):
        b = _joint(own, objs, prm)
        b.set_prepass(mode, delta)
        b.set_report(True)
        b.run()
        out[name] = (b.results(), b.report(), b.stats())
        b.close()
    own.close()
    st = out["trip"][2]
    print("guard trips", st["prepass_guard_trips"], "objects re-run", st["prepass_guard_objects"], "of", len(objs))
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_trips"] > 0
    assert 0 < st["prepass_guard_objects"] < len(objs)          # a PARTIAL re-run: a member is left out of it and keeps the rows it had
    assert _same(out["trip"][0], out["off"][0])
    for key in REPORT_KEYS:
        if key not in ("ray_counts", "m"):
            assert _bits(out["trip"][1][key], out["off"][1][key]), key
    assert np.array_equal(out["trip"][1]["ray_counts"][:, [0, 2]], out["off"][1]["ray_counts"][:, [0, 2]])


def _member_rows(rep, i):
    return [_cut(rep, k, i) if k.startswith(("pt_", "ray_")) else rep[k][i] for k in REPORT_KEYS]


def test_a_good_member_left_out_of_the_rerun_keeps_its_first_run_rows(oracle_decoder, objs):
    """The guard trips where a re-decoded sample is off by half the margin or more.  Each good object's own largest f16 prepass error is read
    from a guarded run of that object alone (no trip at the calibrated margin); a forced margin of their SUM puts the trip point half way
    between them, so exactly one of the two trips.  It is run again with the prepass off and gets fresh rows -- the prepass-off run's --
    while the other GOOD member and the failed one are left out (DSP_STATUS_SKIP in the re-run) and keep every row of the first run,
    which is what the same batch returns with the guard off, bit for bit, band counts included."""
    prm = E.gn_params(num_iterations=N_IT)
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    errs = []
    for i in (0, 1):
        b = _joint(own, [objs[i]], prm)
        b.set_prepass(L.PREPASS_F16)
        b.run()
        st = b.stats()
        assert st["prepass_guard_trips"] == 0 and st["prepass_guard_max_err"] > 0
        errs.append(float(st["prepass_guard_max_err"]))
        b.close()
    tripped, left = int(np.argmax(errs)), int(np.argmin(errs))
    delta = errs[0] + errs[1]
    print("largest prepass errors %s, forced margin %.4g: object %d trips, object %d does not" % (errs, delta, tripped, left))
    assert max(errs) > 1.05 * min(errs)         # the trip point delta / 2 is at least 2.5 % away from either error
    runs = {}
    for name, mode, d, guard in (("guarded", L.PREPASS_F16, delta, True), ("unguarded", L.PREPASS_F16, delta, False), ("off", L.PREPASS_OFF, -1.0, True)):
        b = _joint(own, objs, prm)
        b.set_prepass(mode, d)
        b.set_prepass_guard(guard)
        b.set_report(True)
        b.run()
        runs[name] = (b.results(), b.report(), b.stats())
        b.close()
    own.close()
    st = runs["guarded"][2]
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_objects"] == 1 and runs["unguarded"][2]["prepass_guard_rerun"] == 0
    assert _same(runs["guarded"][0], runs["off"][0])
    for i in (left, 2):         # left out of the re-run: the first run's rows, untouched
        assert all(_bits(np.asarray(x), np.asarray(y)) for x, y in zip(_member_rows(runs["guarded"][1], i), _member_rows(runs["unguarded"][1], i))), i
    fresh, ref = _member_rows(runs["guarded"][1], tripped), _member_rows(runs["off"][1], tripped)
    for k, x, y in zip(REPORT_KEYS, fresh, ref):         # re-run with the prepass off: that run's rows
        assert _bits(np.asarray(x), np.asarray(y)), k


def test_allocation_failure_at_enable_leaves_the_batch_usable(oracle_decoder, objs):
    prm = E.gn_params(num_iterations=2)
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    b = _joint(own, objs, prm)
    b.run()
    good = b.results()
    lib = L.load()
    own.trim()                               # an empty cache: enabling the report has to allocate afresh
    for nth in (0, 3, 6):                    # the first, a middle and the last of the report's seven arrays
        own.fail_alloc(nth)
        assert lib.dsp_batch_report(b._h, 1) == -3 and b"out of device memory" in lib.dsp_last_error(own._h)      # DSP_E_NOMEM
        own.fail_alloc(-1)
        own.trim()
        b.run()                              # usable, with the report off
        assert _same(b.results(), good) and lib.dsp_batch_report_fetch(b._h, *([None] * 7)) == -4
    assert lib.dsp_batch_report(b._h, 2) == -1 and lib.dsp_batch_report(b._h, -1) == -1                              # DSP_E_ARG
    b.set_report(True)
    b.run()
    assert _same(b.results(), good) and b.report()["status"].tolist() == [0, 0, L.OBJ_FEW_SAMPLES]
    b.close()
    own.close()


# ---- the layers above the batch --------------------------------------------------------------------------------------------------------------
def test_engine_keyword_returns_the_report_behind_the_existing_items(eng, objs):
    prm = E.gn_params(num_iterations=3)
    args = ([o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs])
    plain = eng.reconstruct_batch(prm, *args)
    got = eng.reconstruct_batch(prm, *args, report=True)
    assert len(plain) == 4 and len(got) == 5 and _same(plain, got[:4]) and got[4]["status"].tolist() == plain[3].tolist()
    both = eng.reconstruct_batch(prm, *args, posterior="mean", report=True)
    assert len(both) == 6 and _same(plain, both[:4]) and "info_pose" in both[4] and _same(_report_rows(both[5]), _report_rows(got[4]))
    mv = R.multiview_objects()
    margs = ([o["t_cam_obj_init"] for o in mv], [o["views"] for o in mv])
    plain = eng.reconstruct_multiview_batch(prm, *margs)
    got = eng.reconstruct_multiview_batch(prm, *margs, report=True)
    assert len(got) == 5 and _same(plain, got[:4]) and got[4]["view_off"].tolist() == [0, 3, 4] and got[4]["M"].tolist() == [90, 90, 90, 110]
    g = golden("golden_pose_only_8it.npz")
    pargs = ([g["t_co_se3"]], [float(g["scale"])], [g["pts"]], [g["code"]])
    pprm = E.gn_params(pose_only_iterations=8)
    poses = eng.estimate_pose_batch(pprm, *pargs)
    got = eng.estimate_pose_batch(pprm, *pargs, report=True)
    assert isinstance(got, tuple) and len(got) == 2 and np.array_equal(poses, got[0]) and got[1]["M"][0] == got[1]["pt_alive"].sum() < 300


def test_reoptimise_map_writes_the_rows_per_object_id(tmp_path, eng):
    import os
    import sys
    from conftest import ROOT
    from dsp_slam_amd import observations as OBS, synth
    from dsp_slam_amd.map_objects import read_map_objects, write_map_objects
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import reoptimise_map as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    map_dir = tmp_path / "map"
    (map_dir / "observations").mkdir(parents=True)
    made, objs = {}, []
    for i, (n_s, n_b) in enumerate(((120, 40), (97, 35), (150, 30))):
        o = synth.make_object(7100 + i, n_surface=n_s, n_background=n_b)
        made[5 * i + 2] = o
        objs.append(dict(id=5 * i + 2, pose=o["t_cam_obj_init"].astype(np.float64), code=np.zeros(64, np.float32)))
        if i != 1:                      # object 7 has no observation: no rows
            np.savez(map_dir / "observations" / ("%d.npz" % (5 * i + 2)), pts=o["pts"], rays=o["rays"], depth=o["depth"], t_world_cam=np.eye(4))
    write_map_objects(str(map_dir / "MapObjects.txt"), objs)
    objs = read_map_objects(str(map_dir / "MapObjects.txt"))
    obs = tool.load_observations(str(map_dir), objs)
    prm = E.gn_params(num_iterations=3)
    plain, st0 = tool.reoptimise([eng], prm, objs, obs, 64)
    out, st = tool.reoptimise([eng], prm, objs, obs, 64, report=True)
    assert st0["report"] is None and np.array_equal(st0["packed"], st["packed"])
    rows = st["report"]
    assert sorted({k.split("/")[0] for k in rows}) == ["12", "2"]
    assert rows["2/pt_sdf"].shape == (120,) and rows["12/pt_sdf"].shape == (150,) and rows["12/ray_hit"].shape == (180,) and rows["2/status"].tolist() == [0]
    np.savez(str(tmp_path / "rows.npz"), **rows)
    back = np.load(str(tmp_path / "rows.npz"))
    one = {k.split("/")[1]: back[k] for k in back.files if k.startswith("12/")}
    assert OBS.point_outliers(one, 0.5)[0].sum() == 0 and OBS.silhouette_disagreement(one)["fg_miss"].shape == (1,)
    # the command-line flag: the same keys, written by the tool itself (the config's 10 iterations, a decoder loaded from the on-disk format)
    import json
    import runpy
    from dsp_slam_amd import fixtures
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    cfg["DeepSDF_DIR"] = fixtures.materialize_decoder_dir("cars", str(tmp_path / "cars_64"))
    cfg.setdefault("data_type", "KITTI")
    with open(str(tmp_path / "cfg.json"), "w") as f:
        json.dump(cfg, f)
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    old_argv, old_mods = sys.argv, [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]
    for m in old_mods:
        del sys.modules[m]
    sys.path.insert(0, pkg)
    sys.argv = ["reoptimise_map.py", "--config", str(tmp_path / "cfg.json"), "--map_dir", str(map_dir), "--gpus", "1", "--report", str(tmp_path / "cli.npz")]
    try:
        runpy.run_path(os.path.join(ROOT, "tools", "reoptimise_map.py"), run_name="__main__")
    finally:
        sys.argv = old_argv
        sys.path.remove(pkg)
        for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
            del sys.modules[m]
    cli = np.load(str(tmp_path / "cli.npz"))
    assert sorted(cli.files) == sorted(rows) and cli["2/pt_sdf"].shape == (120,) and np.isfinite(cli["12/ray_depth"]).all() and cli["12/status"].tolist() == [0]
