"""GPU: the mask of unknowns (dsp_batch_unknowns, include/dsp_gn.h) through every layer.

  1. off equals plain: NULL, a mask of ones and a mask set then cleared return the plain run's results, traces and launch counts bit for
     bit (joint; pose-only with the inlier filter; three views);
  2. frozen means untouched: traced dx exactly 0.0 at frozen entries in every iteration, frozen code entries keep their bits, with the pose
     frozen t_obj_cam and the depth samples keep theirs and the result pose is that of a one-iteration run; with nothing live the state
     does not move and `loss` is the loss at the start state;
  3. iteration 0 shares its linearisation with the plain run: live x live of H and live b bit-equal, identity and 0 elsewhere;
  4. every iteration against the conditioned fp64 reference (tests/unknowns_ref.py) at the device's own traced states on its own sets,
     through gn_metric.check_against_fp64 with TAU_H / TAU_B / TAU_SOLVE as they stand (pair=None);
  5. upright: with w_x, w_z frozen and k4 = 0 the object's up axis keeps its direction to fp32 round-off, where the plain run tilts;
  6. independence: masked and unmasked objects of one batch do not see each other;
  7. with the convergence rule, step control, the prior, the posterior, observation weights, the report, the f16 compute mode, a partial
     re-run after a prepass-guard trip, and a 32-D decoder;
  8. errors; 9. tools/reoptimise_map.py --unknowns.

Every comparison prints its figure before it asserts; the figures of an MI355X run are in profiles/unknowns.md.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gn_metric as M
import multiview_metric as X
import posterior_ref as R
import unknowns_ref as U
import weights_ref as W
from conftest import ROOT, golden, parity_log
from dsp_slam_amd import _lib as L, engine as E, synth
from oracle import dsp_oracle as O
from test_gpu_weights import _ragged_objects, _same, _weights

pytestmark = pytest.mark.gpu
F32 = np.float32
TRACE_KEYS = ("H", "b", "dx", "V", "K", "t_obj_cam", "code", "depths")
LAUNCHES = ("n_mlp_fwd_launches", "n_mlp_jac_launches", "n_mlp_prepass_launches")
N_IT = 3
U8P = C.POINTER(C.c_uint8)


def _random_mask(seed, n=71):
    m = (np.random.default_rng(seed).random(n) >= 0.5).astype(np.uint8)
    m[0], m[1] = 1, 0
    return m


# the masks of tests 2 and 3, named by what they FREEZE
FROZEN = {"code": E.unknowns_mask("pose"), "pose": E.unknowns_mask("code"), "scale": 1 - E.unknowns_mask("scale"),
          "w_xz": E.unknowns_mask(["translation", "yaw", "scale", "code"]), "random": _random_mask(31)}


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _codes(objs, seed=9):
    """Non-zero start codes: a frozen code entry that is zero would not show an update that adds to it."""
    rng = np.random.default_rng(seed)
    return [(0.05 * rng.standard_normal(64)).astype(F32) for _ in objs]


def _joint(eng, objs, prm, trace=True, codes=None):
    return eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                     _codes(objs) if codes is None else codes, trace=trace)


def _run(b, n_it, keys=TRACE_KEYS):
    b.run()
    out = list(b.results())
    traces = [b.trace(e) for e in range(n_it)]
    for tr in traces:
        out += [tr[k] for k in keys]
    return out, traces


def _launches(b):
    return [b.stats()[k] for k in LAUNCHES]


@pytest.fixture(scope="module")
def plain(eng):
    """The plain run of the three ragged objects every test compares with (made once)."""
    objs = _ragged_objects()
    prm = E.gn_params(num_iterations=N_IT)
    b = _joint(eng, objs, prm)
    out, traces = _run(b, N_IT)
    launches = _launches(b)
    b.close()
    assert out[3].tolist() == [0, 0, 0]
    return dict(objs=objs, prm=prm, out=out, traces=traces, launches=launches)


# ---- 1. off equals plain ---------------------------------------------------------------------------------------------------------------
def test_off_joint_is_the_plain_run(eng, plain):
    b = _joint(eng, plain["objs"], plain["prm"])
    for live in (None, np.ones((3, 71), np.uint8), np.ones(71, np.uint8), ["all"], ["pose", "code"]):
        b.set_unknowns(live)
        assert _same(plain["out"], _run(b, N_IT)[0]) and _launches(b) == plain["launches"]
    b.set_unknowns(["pose"])
    masked = _run(b, N_IT)[0]
    assert masked[3].tolist() == [0, 0, 0] and not _same(plain["out"], masked)
    b.set_unknowns(None)                                    # set, then cleared
    assert _same(plain["out"], _run(b, N_IT)[0]) and _launches(b) == plain["launches"]
    b.close()


def test_off_pose_only_with_the_inlier_filter_is_the_plain_run(eng):
    g = golden("golden_pose_only_8it.npz")
    prm = E.gn_params(pose_only_iterations=8)
    b = eng.pose_batch(prm, [g["t_co_se3"]], [float(g["scale"])], [g["pts"]], [g["code"]], trace=True)
    keys = ("H", "b", "dx", "K", "t_obj_cam")
    want = _run(b, 8, keys)[0]
    assert int(b.trace(7)["K"][0]) < g["pts"].shape[0]          # the filter dropped points
    for live in (np.ones((1, 6), np.uint8), ["pose"], None):
        b.set_unknowns(live)
        assert _same(want, _run(b, 8, keys)[0])
    b.set_unknowns(["translation", "yaw"])
    assert not _same(want, _run(b, 8, keys)[0])
    b.set_unknowns()
    assert _same(want, _run(b, 8, keys)[0])
    b.close()


def test_off_three_views_is_the_plain_run(eng):
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
        return out, _launches(b)
    want = run()
    for live in (np.ones((1, 71), np.uint8), None):
        b.set_unknowns(live)
        got = run()
        assert _same(want[0], got[0]) and want[1] == got[1]
    b.set_unknowns(["code"])
    assert not _same(want[0], run()[0])
    b.set_unknowns(None)
    got = run()
    assert _same(want[0], got[0]) and want[1] == got[1]
    b.close()


# ---- 2. frozen means untouched; 3. iteration 0 shares its linearisation with the plain run ----------------------------------------------
@pytest.mark.parametrize("name", sorted(FROZEN))
def test_frozen_entries_are_untouched_and_iteration_0_is_the_plain_linearisation(eng, plain, name):
    live = FROZEN[name]
    lv = live.astype(bool)
    objs, prm = plain["objs"], plain["prm"]
    b = _joint(eng, objs, prm)
    b.set_unknowns(live)
    out, traces = _run(b, N_IT)
    assert out[3].tolist() == [0, 0, 0]
    worst = max(float(np.abs(tr["dx"][:, ~lv]).max()) for tr in traces)
    moved = max(float(np.abs(tr["dx"][:, lv]).max()) for tr in traces)
    print("frozen %s: %d live entries, largest |dx| at a frozen entry %g, at a live entry %.3g" % (name, lv.sum(), worst, moved))
    for e, tr in enumerate(traces):
        assert np.array_equal(tr["dx"][:, ~lv], np.zeros((3, int((~lv).sum())), F32)), "iteration %d" % e
        assert np.array_equal(tr["code"][:, ~lv[7:]].view(np.uint32), traces[0]["code"][:, ~lv[7:]].view(np.uint32)), "iteration %d" % e
    assert moved > 1e-4
    assert np.array_equal(out[1][:, ~lv[7:]].view(np.uint32), traces[0]["code"][:, ~lv[7:]].view(np.uint32))          # the result's code too
    if lv[7:].any():
        assert not np.array_equal(out[1][:, lv[7:]], traces[0]["code"][:, lv[7:]])
    if not lv[:7].any():
        for e, tr in enumerate(traces):
            assert np.array_equal(tr["t_obj_cam"].view(np.uint32), traces[0]["t_obj_cam"].view(np.uint32)), "iteration %d" % e
            assert np.array_equal(tr["depths"].view(np.uint32), traces[0]["depths"].view(np.uint32)), "iteration %d" % e
        b.set_iterations(1)
        b.run()
        assert np.array_equal(out[0].view(np.uint32), b.results()[0].view(np.uint32))          # the pose of an N-iteration run is that of one iteration
    b.close()
    # 3. iteration 0: the masked system is the plain run's on live x live, identity and 0 elsewhere
    h, rhs = traces[0]["H"], traces[0]["b"]
    h0, rhs0 = plain["traces"][0]["H"], plain["traces"][0]["b"]
    n_fz = int((~lv).sum())
    for i in range(3):
        assert np.array_equal(h[i][np.ix_(lv, lv)].view(np.uint32), h0[i][np.ix_(lv, lv)].view(np.uint32))
        assert np.array_equal(rhs[i][lv].view(np.uint32), rhs0[i][lv].view(np.uint32))
        assert np.array_equal(h[i][np.ix_(~lv, ~lv)], np.eye(n_fz, dtype=F32)) and not h[i][np.ix_(lv, ~lv)].any() and not h[i][np.ix_(~lv, lv)].any()
        assert not rhs[i][~lv].any()
    for k in ("V", "K", "t_obj_cam", "code", "depths", "set_sums"):
        assert np.array_equal(traces[0][k], plain["traces"][0][k]), k


def test_nothing_live_evaluates_and_moves_nothing(eng, plain):
    objs, prm = plain["objs"], plain["prm"]
    b = _joint(eng, objs, prm)
    b.set_unknowns([])
    out, traces = _run(b, N_IT)
    b.set_iterations(1)
    one, _ = _run(b, 1)
    b.close()
    assert out[3].tolist() == [0, 0, 0]
    for tr in traces:
        assert not tr["dx"].any() and np.array_equal(tr["H"], np.tile(np.eye(71, dtype=F32), (3, 1, 1))) and not tr["b"].any()
        for k in ("t_obj_cam", "code", "depths", "V", "K", "set_sums"):
            assert np.array_equal(tr[k], traces[0][k]), k
    print("nothing live: loss after %d iterations %s, after one %s, plain first linearisation loss from the same state" % (N_IT, out[2], one[2]))
    assert np.array_equal(out[0].view(np.uint32), one[0].view(np.uint32)) and np.array_equal(out[1], traces[0]["code"])
    assert np.array_equal(out[2].view(np.uint32), one[2].view(np.uint32))          # the loss at the start state
    # ... and a plain one-iteration run reports that loss too (its loss is the loss of its first linearisation)
    c = _joint(eng, objs, E.gn_params(num_iterations=1))
    c.run()
    assert np.array_equal(c.results()[2].view(np.uint32), out[2].view(np.uint32))
    c.close()


def test_pose_only_frozen_entries(eng):
    g = golden("golden_pose_only_8it.npz")
    prm = E.gn_params(pose_only_iterations=8)
    b = eng.pose_batch(prm, [g["t_co_se3"]], [float(g["scale"])], [g["pts"]], [g["code"]], trace=True)
    live = E.unknowns_mask(["translation", "yaw"], pose_only=True)
    lv = live.astype(bool)
    b.set_unknowns(live)
    b.run()
    traces = [b.trace(e) for e in range(8)]
    for tr in traces:
        assert np.array_equal(tr["dx"][0][~lv], np.zeros(2, F32)) and np.abs(tr["dx"][0][lv]).max() > 0
        assert np.array_equal(tr["H"][0][np.ix_(~lv, ~lv)], np.eye(2, dtype=F32)) and not tr["H"][0][np.ix_(lv, ~lv)].any() and not tr["b"][0][~lv].any()
    b.set_unknowns(np.zeros(6, np.uint8))                   # all six frozen: the pose keeps its bits
    b.run()
    assert all(np.array_equal(b.trace(e)["t_obj_cam"].view(np.uint32), b.trace(0)["t_obj_cam"].view(np.uint32)) for e in range(8))
    assert not any(b.trace(e)["dx"].any() for e in range(8))
    b.close()


# ---- 4. every iteration against the conditioned fp64 reference --------------------------------------------------------------------------
WORST = {}


def _note(kind, rec):
    WORST[kind] = max(WORST.get(kind, 0.0), max(v for k, v in rec.items() if k.startswith("dev_") and k != "dev_solve"))
    print("worst scaled error so far (%s): %.3e" % (kind, WORST[kind]))


def _check_joint_iterations(eng, dec, objs, prm, oprm, live, codes, label, pw=None, rw=None):
    """A masked run of `objs`, then every iteration once more from its traced state: each object's system against the conditioned fp64
    reference on the device's own sets there."""
    live = np.broadcast_to(np.asarray(live, np.uint8), (len(objs), 71))
    n_d, n_it = oprm.num_depth_samples, prm.num_iterations
    b = _joint(eng, objs, prm, codes=codes)
    b.set_unknowns(live)
    if pw is not None or rw is not None:
        b.set_observation_weights(pw, rw)
    b.run()
    assert b.results()[3].tolist() == [0] * len(objs)
    traces = [b.trace(e) for e in range(n_it)]
    for e, tr in enumerate(traces):
        b.set_start_state(tr["t_obj_cam"], tr["code"], tr["depths"])
        b.set_iterations(1)
        b.run()
        tr1 = b.trace(0)
        assert all(np.array_equal(tr1[k], tr[k]) for k in ("H", "b", "dx", "V", "K")), "the re-run from the traced state does not reproduce the traced system"
        for i, o in enumerate(objs):
            m, _, deds = b.debug_samples(i, o["rays"].shape[0], n_d)
            sets = W.device_sets(m, deds)
            assert sets["valid"][0].shape[0] == int(tr["V"][i]) and sets["kept"][0].shape[0] == int(tr["K"][i])
            lin = W.linearise(dec, oprm, o["pts"], o["rays"], o["depth"], tr["t_obj_cam"][i], tr["code"][i], tr["depths"][i][:n_d], sets,
                              None if pw is None else pw[i], None if rw is None else rw[i])
            ref = U.condition(lin, live[i])
            dev = dict(H=tr["H"][i], b=tr["b"][i], dx=tr["dx"][i])
            what = "%s iteration %d object %d" % (label, e, i)
            print("%s (%d live): V %d K %d: %s" % (what, live[i].sum(), tr["V"][i], tr["K"][i], M.flat(M.scaled_errors(dev, ref, oprm.k4))))
            rec = M.check_against_fp64(dev, ref, oprm.k4, what=what)
            _note(label, rec)
            parity_log(kind="unknowns_fp64", case=label, iteration=e, object=i, **rec)
    b.close()


@pytest.mark.parametrize("name,k4", [("code", 1e7), ("scale", 1e7), ("w_xz", 0.0)])
def test_joint_systems_against_the_conditioned_fp64(eng, oracle_decoder, plain, name, k4):
    prm, oprm = E.gn_params(num_iterations=N_IT, k4=k4), O.GNParams(num_iterations=1, k4=k4)
    _check_joint_iterations(eng, oracle_decoder, plain["objs"], prm, oprm, FROZEN[name], None, "joint, %s frozen" % name)


def test_pose_only_systems_against_the_conditioned_fp64(eng, oracle_decoder):
    g = golden("golden_pose_only_8it.npz")
    pts = g["pts"]
    prm = E.gn_params(pose_only_iterations=8)
    live6 = E.unknowns_mask(["translation", "yaw"], pose_only=True)
    live = np.ones(71, np.uint8)
    live[:6] = live6
    b = eng.pose_batch(prm, [g["t_co_se3"]], [float(g["scale"])], [pts], [g["code"]], trace=True)
    b.set_unknowns(live6)
    b.set_report(True)
    b.run()
    alive = b.report()["pt_alive"]
    traces = [b.trace(e) for e in range(8)]
    b.close()
    print("pose-only, yaw + translation live: %d of %d points alive behind the filter" % (alive.sum(), pts.shape[0]))
    assert 0 < alive.sum() <= pts.shape[0]
    for e, tr in enumerate(traces):
        al = None if e <= 4 else alive                        # the filter runs behind iteration 4
        lin = W.pose_only(oracle_decoder, pts, tr["t_obj_cam"][0], g["code"], None, al)
        assert int(tr["K"][0]) == (pts.shape[0] if al is None else int(alive.sum()))
        ref = U.condition(lin, live)
        dev = W.embed6(tr["H"][0], tr["b"][0], tr["dx"][0])
        print("pose-only iteration %d: %s" % (e, M.flat(M.scaled_errors(dev, ref, 0.0))))
        _note("pose_only", M.check_against_fp64(dev, ref, 0.0, what="masked pose-only iteration %d" % e))
        assert not tr["dx"][0][[3, 5]].any()


def test_two_multiview_objects_with_their_own_masks_against_the_conditioned_fp64(eng, oracle_decoder):
    case = X.case_ragged()
    objs = case["objects"][:2]                                  # two views, one view
    views = [v for o in objs for v in o["views"]]
    off = np.concatenate([[0], np.cumsum([len(o["views"]) for o in objs])]).astype(int)
    live = np.stack([FROZEN["code"], FROZEN["w_xz"]])
    prm, oprm = E.gn_params(num_iterations=case["n_it"], **X.HYPER), X.oracle_params(case)
    n_d = case["n_depth"]
    b = eng.multiview_batch(prm, [o["t"] for o in objs], [o["views"] for o in objs], _codes(objs), trace=True)
    b.set_unknowns(live)
    b.run()
    assert b.results()[3].tolist() == [0, 0]
    traces = [(b.trace(e), b.trace_views(e)) for e in range(case["n_it"])]
    for e, (tr, tv) in enumerate(traces):
        b.set_start_state(tr["t_obj_cam"], tr["code"], tv["depths"])
        b.set_iterations(1)
        b.run()
        tr1, tv1 = b.trace(0), b.trace_views(0)
        assert all(np.array_equal(tr1[k], tr[k]) for k in ("H", "b", "dx", "V", "K")) and np.array_equal(tv1["set_sums"], tv["set_sums"])
        for i, o in enumerate(objs):
            rows = range(off[i], off[i + 1])
            sets = []
            for k in rows:
                m, _, deds = b.debug_samples(k, views[k]["rays"].shape[0], n_d)
                sets.append(W.device_sets(m, deds))
            lin = W.linearise_multiview(oracle_decoder, oprm, o["views"], tr["t_obj_cam"][i], tr["code"][i], [tv["depths"][k][:n_d] for k in rows], sets)
            assert lin["K_views"] == [int(tv["K"][k]) for k in rows]
            ref = U.condition(lin, live[i])
            dev = dict(H=tr["H"][i], b=tr["b"][i], dx=tr["dx"][i])
            print("multi-view iteration %d object %d (%d views, %d live): %s" % (e, i, len(o["views"]), live[i].sum(), M.flat(M.scaled_errors(dev, ref, oprm.k4))))
            _note("multiview", M.check_against_fp64(dev, ref, oprm.k4, what="masked multi-view iteration %d object %d" % (e, i)))
            lv = live[i].astype(bool)
            assert np.array_equal(tr["dx"][i][~lv], np.zeros(int((~lv).sum()), F32))
    b.close()


# ---- 5. upright ------------------------------------------------------------------------------------------------------------------------
def _up(t):
    """The normalised second row of a matrix's 3 x 3 block: the object's up axis in the camera frame."""
    r = np.asarray(t, np.float64)[1, :3]
    return r / np.linalg.norm(r)


def _exp_rot_scale64(dx):
    """e^sigma R(w) of the Sim(3) exponential in float64 (Rodrigues; the translation does not reach the 3 x 3 block of a left update)."""
    w, s = np.asarray(dx[3:6], np.float64), float(dx[6])
    th = float(np.linalg.norm(w))
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    a, c = (1.0, 0.5) if th < 1e-12 else (np.sin(th) / th, (1 - np.cos(th)) / th ** 2)
    return np.exp(s) * (np.eye(3) + a * k + c * (k @ k))


@pytest.mark.parametrize("start", ["upright", "tilted"])
def test_upright_with_wx_wz_frozen_and_k4_zero(eng, start):
    """With w = (0, w_y, 0) Rodrigues gives R[1, :] = e_y exactly, so the update multiplies the second row of t_obj_cam[:3, :3] by
    e^sigma: its direction -- the object's up axis in the camera frame -- moves by the roundings of that multiply alone.  The limit
    after e iterations is 4 x the sum over them of the distance the SAME update, evaluated in float64 from the traced fp32 matrix and the
    traced dx and rounded once to fp32, moves the normalised row (not below one half ulp of a unit entry, 2^-24, per iteration)."""
    o = _ragged_objects()[0]                                    # seed 710: the CPU oracle's plain run with k4 = 0 tilts by 0.074 in its first step
    if start == "tilted":
        # the synthetic start pose is exactly upright (the row is (0, -1 / s, 0): scaling cannot turn it); rotated by 0.05 rad about the
        # object's x axis the row has two non-zero entries, and the frozen run has to keep THAT direction
        c, sn = np.cos(0.05), np.sin(0.05)
        rx = np.array([[1, 0, 0, 0], [0, c, -sn, 0], [0, sn, c, 0], [0, 0, 0, 1]], np.float64)
        o = dict(o, t_cam_obj_init=(o["t_cam_obj_init"].astype(np.float64) @ rx).astype(F32))
    n_it = 4
    prm = E.gn_params(num_iterations=n_it, k4=0.0)
    rows = {}
    for name, live in (("frozen", FROZEN["w_xz"]), ("plain", None)):
        b = _joint(eng, [o], prm)
        b.set_unknowns(live)
        b.run()
        assert b.results()[3].tolist() == [0]
        rows[name] = [b.trace(e) for e in range(n_it)]
        b.close()
    tr = rows["frozen"]
    limit, acc, worst_ratio = [0.0], 0.0, 0.0
    for e in range(n_it - 1):
        t = tr[e]["t_obj_cam"][0].astype(np.float64)
        nxt = (_exp_rot_scale64(prm.lr * tr[e]["dx"][0].astype(np.float64)) @ t[:3, :3]).astype(F32)
        acc += max(float(np.linalg.norm(_up(nxt) - _up(t))), 2.0 ** -24)
        limit.append(4 * acc)
    for e in range(n_it):
        d = float(np.linalg.norm(_up(tr[e]["t_obj_cam"][0]) - _up(tr[0]["t_obj_cam"][0])))
        dp = float(np.linalg.norm(_up(rows["plain"][e]["t_obj_cam"][0]) - _up(rows["plain"][0]["t_obj_cam"][0])))
        print("upright (%s start) iteration %d: |up - up_0| with w_x, w_z frozen %.3e (limit %.3e), plain run %.3e; yaw step %.3e" % (
            start, e, d, limit[e], dp, float(tr[e]["dx"][0][4])))
        assert d <= limit[e]
        worst_ratio = max(worst_ratio, dp / max(limit[e], 1e-300)) if e else 0.0
    WORST["upright_plain_over_limit_" + start] = worst_ratio
    assert worst_ratio > 1.0, "the plain run does not tilt beyond the limit: the test shows nothing"
    assert max(abs(float(t["dx"][0][4])) for t in tr) > 1e-4          # the yaw did move


# ---- 6. independence -------------------------------------------------------------------------------------------------------------------
def test_masked_and_plain_objects_of_one_batch_do_not_see_each_other(eng, plain):
    objs, prm = plain["objs"], plain["prm"]
    live = np.ones((3, 71), np.uint8)
    live[1] = FROZEN["random"]
    b = _joint(eng, objs, prm)
    b.set_unknowns(live)
    out, _ = _run(b, N_IT)
    b.close()
    codes = _codes(objs)
    s = _joint(eng, [objs[1]], prm, codes=[codes[1]])
    s.set_unknowns(FROZEN["random"])
    single, _ = _run(s, N_IT)
    s.close()
    for a, p_, q in zip(out, plain["out"], single):
        assert np.array_equal(a[0], p_[0], equal_nan=True) and np.array_equal(a[2], p_[2], equal_nan=True)
        assert np.array_equal(a[1], q[0], equal_nan=True)
    assert not np.array_equal(out[0][1], plain["out"][0][1])


# ---- 7. with the other features --------------------------------------------------------------------------------------------------------
def test_with_the_convergence_rule_an_object_with_nothing_live_stops_at_min_iterations(eng, plain):
    objs = plain["objs"]
    n_it = 5
    live = np.ones((3, 71), np.uint8)
    live[1] = 0
    b = _joint(eng, objs, E.gn_params(num_iterations=n_it))
    b.set_unknowns(live)
    b.set_convergence(1e-12, 1e-12, 2)                      # tolerances no moving object meets
    b.run()
    used, res = b.iterations_used(), b.results()
    print("convergence rule, object 1 with nothing live: iterations used", used)
    assert used.tolist() == [n_it, 2, n_it] and res[3].tolist() == [0, 0, 0]
    # frozen entries block no stop: with the code frozen only the pose tolerance decides
    b.set_unknowns(["pose"])
    b.set_convergence(float("inf"), 1e-12, 1)
    b.run()
    assert b.iterations_used().tolist() == [1, 1, 1]
    b.set_unknowns(None)
    b.run()
    assert b.iterations_used().tolist() == [n_it] * 3
    b.close()


def test_with_step_control(eng, plain):
    o = plain["objs"][0]
    n_it = 8
    live = FROZEN["random"]
    lv = live.astype(bool)
    b = _joint(eng, [o], E.gn_params(num_iterations=n_it, lr=4.0))
    b.set_unknowns(live)
    b.set_step_control(1.0, 10.0, 0.1, 1.0, float("inf"))
    b.run()
    log = b.step_log()
    traces = [b.trace(e) for e in range(n_it)]
    res = b.results()
    b.close()
    print("step control with a mask: decisions %s lambdas %s" % (log["decision"][:, 0], log["lambda"][:, 0]))
    assert res[3].tolist() == [0] and log["decision"].shape == (n_it, 1) and (log["decision"] != 0).all()
    assert (log["decision"] == 2).any(), "no step was rejected: choose another learning rate"
    for e, tr in enumerate(traces):
        assert np.array_equal(tr["dx"][0][~lv], np.zeros(int((~lv).sum()), F32)), "iteration %d" % e
        assert np.array_equal(np.diag(tr["H"][0])[~lv], np.ones(int((~lv).sum()), F32))          # lambda (>= 1 here) is not on a frozen diagonal
        assert np.array_equal(tr["code"][0][~lv[7:]].view(np.uint32), traces[0]["code"][0][~lv[7:]].view(np.uint32))
    assert np.array_equal(res[1][0][~lv[7:]].view(np.uint32), traces[0]["code"][0][~lv[7:]].view(np.uint32))


def test_with_the_prior(eng, plain):
    o = plain["objs"][0]
    live = FROZEN["random"]
    lv = live.astype(bool)
    prm = E.gn_params(num_iterations=2)
    b = _joint(eng, [o], prm)
    b.set_posterior(2, "sum")
    b.run()
    rec = b.posterior()
    assert rec["status"].tolist() == [0]
    b.set_posterior(0, "sum")
    h = {}
    for name, mask, prior in (("plain", None, False), ("plain_prior", None, True), ("masked", live, False), ("masked_prior", live, True)):
        b.set_unknowns(mask)
        if prior:
            b.set_prior(rec["t_obj_cam"], rec["code"], 1e-3 * rec["Lambda"])
        else:
            b.set_prior()
        b.run()
        assert b.results()[3].tolist() == [0]
        h[name] = b.trace(0)["H"][0].astype(np.float64)
        if prior:
            pr = b.prior_residual()
            assert pr["e"].shape == (1, 71) and np.isfinite(pr["e"]).all() and np.isfinite(pr["chi2"]).all() and pr["chi2"][0] > 0
    b.close()
    d_plain, d_masked = h["plain_prior"] - h["plain"], h["masked_prior"] - h["masked"]
    assert not d_masked[~lv].any() and not d_masked[:, ~lv].any()                      # nothing of the prior in a frozen row or column
    tol = 4 * np.maximum(M.ulp32(h["plain_prior"]), M.ulp32(h["plain"]))
    err = np.abs(d_masked - d_plain)[np.ix_(lv, lv)]
    print("prior block, masked against plain on live x live: worst difference %.3e (4 ulp32 there: %.3e), largest entry %.3e" % (
        err.max(), tol[np.ix_(lv, lv)].flat[err.argmax()], np.abs(d_plain).max()))
    assert np.all(err <= tol[np.ix_(lv, lv)]) and np.abs(d_plain[np.ix_(lv, lv)]).max() > 0


@pytest.mark.parametrize("name", ["random", "code", "pose"])
def test_with_the_posterior(eng, plain, name):
    objs = plain["objs"][:2]
    live = FROZEN[name]
    lv = live.astype(bool)
    prm = E.gn_params(num_iterations=N_IT)
    b = _joint(eng, objs, prm)
    b.set_unknowns(live)
    b.set_posterior(2, "mean")
    b.run()
    rec = b.posterior()
    res = b.results()
    b.set_posterior(1, "mean")
    b.run()
    rec1 = b.posterior()
    b.close()
    assert rec["status"].tolist() == [0, 0] and res[3].tolist() == [0, 0]
    for k in ("status", "info_pose", "cov_pose", "var_code", "loss"):
        assert np.array_equal(rec[k], rec1[k]), k              # level 1 holds the same marginals
    # the record's state is the returned state: a plain one-iteration batch from it traces H = Lambda + damping on live x live
    c = _joint(eng, objs, E.gn_params(num_iterations=1))
    c.set_start_state(rec["t_obj_cam"], rec["code"], rec["depths"])
    c.run()
    h_plain = c.trace(0)["H"]
    g_plain = c.trace(0)["b"]
    c.close()
    pl, cl = lv[:7], lv[7:]
    for i in range(2):
        lam, g = rec["Lambda"][i], rec["g"][i]
        assert not lam[~lv].any() and not lam[:, ~lv].any() and not g[~lv].any() and np.array_equal(lam, lam.T)
        assert np.array_equal(R.with_damping(lam, prm.s_damp)[np.ix_(lv, lv)].astype(F32), h_plain[i][np.ix_(lv, lv)])
        assert np.array_equal(g[lv].astype(F32), g_plain[i][lv])
        info, cov, var = rec["info_pose"][i], rec["cov_pose"][i], rec["var_code"][i]
        assert not info[~pl].any() and not info[:, ~pl].any() and not cov[~pl].any() and not cov[:, ~pl].any() and not var[~cl].any()
        emu, ref = U.posterior(lam, live), U.posterior(lam, live, refined=True)
        idx = np.nonzero(lv)[0]                                 # the same live block through plain float64 LAPACK: the bound of tests/test_gpu_posterior.py
        inv = np.linalg.inv(lam[np.ix_(idx, idx)])
        p = int(pl.sum())
        lap = dict(cov_pose=inv[:p, :p], var_code=np.diag(inv)[p:], info_pose=np.linalg.inv(inv[:p, :p]) if p else np.zeros((0, 0)))
        assert emu["status"] == 0
        for key, dv in (("cov_pose", cov[np.ix_(pl, pl)]), ("var_code", var[cl]), ("info_pose", info[np.ix_(pl, pl)])):
            r = ref[key][np.ix_(pl, pl)] if key != "var_code" else ref[key][cl]
            e_ = emu[key][np.ix_(pl, pl)] if key != "var_code" else emu[key][cl]
            if r.size == 0:                                     # (no live entry of this kind: the zeros are asserted above)
                continue
            e_dev, e_lap, e_emu = R.rel_err(dv, r), R.rel_err(lap[key], r), R.rel_err(dv, e_)
            print("posterior, %s frozen, object %d, %s: device error %.2e, lapack %.2e, against the restated elimination %.2e" % (name, i, key, e_dev, e_lap, e_emu))
            assert e_dev <= max(8 * e_lap, 1e-13), key
            if key != "var_code":
                assert e_emu <= 1e-12, key
            WORST["posterior_" + key] = max(WORST.get("posterior_" + key, 0.0), e_dev)
        if name == "code":
            assert not var.any() and info[np.ix_(pl, pl)].any()
        if name == "pose":
            assert not info.any() and not cov.any() and np.all(var[cl] > 0)


def test_with_observation_weights(eng, oracle_decoder, plain):
    objs = plain["objs"][:2]
    rng = np.random.default_rng(41)
    pw = [_weights(rng, o["pts"].shape[0]) for o in objs]
    rw = [_weights(rng, o["rays"].shape[0]) for o in objs]
    prm, oprm = E.gn_params(num_iterations=2), O.GNParams(num_iterations=1)
    _check_joint_iterations(eng, oracle_decoder, objs, prm, oprm, np.stack([FROZEN["random"], FROZEN["scale"]]), None, "weights + mask", pw, rw)


def test_with_the_report(eng, plain):
    """The masked run's report rows are those of a plain batch evaluated AT the masked run's returned state (step control's one-iteration
    run evaluates its start state and applies no step)."""
    objs, prm = plain["objs"], plain["prm"]
    b = _joint(eng, objs, prm)
    b.set_unknowns(FROZEN["code"])
    b.set_report(True)
    b.set_posterior(2, "mean")                              # (its record holds the returned state)
    b.run()
    rep, rec = b.report(), b.posterior()
    b.close()
    c = _joint(eng, objs, E.gn_params(num_iterations=1))
    c.set_start_state(rec["t_obj_cam"], rec["code"], rec["depths"])
    c.set_step_control(0.0, 10.0, 0.1, 1.0, float("inf"))
    c.set_report(True)
    c.run()
    want = c.report()
    c.close()
    assert rep["status"].tolist() == [0, 0, 0]
    for k in sorted(want):
        assert np.array_equal(rep[k], want[k], equal_nan=True), k


def test_in_the_low_precision_compute_mode(eng, plain):
    objs, prm = plain["objs"], plain["prm"]
    codes = _codes(objs)

    def run(live):
        b = _joint(eng, objs, prm, trace=False, codes=codes)
        b.set_compute(L.COMPUTE_F16)
        b.set_lp_small_batches(1)
        b.set_unknowns(live)
        b.run()
        res = b.results()
        b.close()
        return res
    free, frozen = run(None), run(FROZEN["code"])
    assert free[3].tolist() == [0, 0, 0] and frozen[3].tolist() == [0, 0, 0]
    assert np.array_equal(frozen[1].view(np.uint32), np.stack(codes).view(np.uint32)) and not np.array_equal(free[1], np.stack(codes))
    assert not np.array_equal(frozen[0], free[0])
    assert _same(free, run(np.ones((3, 71), np.uint8)))


def test_a_partial_rerun_after_a_guard_trip_keeps_the_mask(oracle_decoder, plain):
    """A forced bf16 margin of 2e-5 trips the prepass guard (tests/test_gpu_weights.py): the tripped objects run again with the prepass off.
    With a mask set, every object's result row is the masked prepass-off run's, bit for bit."""
    objs = plain["objs"]
    prm = E.gn_params(num_iterations=3)
    codes = _codes(objs)
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    out = {}
    for name, mode, delta, live in (("off", L.PREPASS_OFF, -1.0, FROZEN["code"]), ("trip", L.PREPASS_BF16, 2e-5, FROZEN["code"]), ("plain", L.PREPASS_OFF, -1.0, None)):
        b = _joint(own, objs, prm, trace=False, codes=codes)
        b.set_prepass(mode, delta)
        b.set_unknowns(live)
        b.run()
        out[name] = (b.results(), b.stats())
        b.close()
    own.close()
    st = out["trip"][1]
    print("masked, guard trips", st["prepass_guard_trips"], "objects re-run", st["prepass_guard_objects"], "of", len(objs))
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_trips"] > 0 and st["prepass_guard_objects"] > 0
    assert out["off"][0][3].tolist() == [0, 0, 0]
    assert _same(out["trip"][0], out["off"][0]) and not _same(out["off"][0], out["plain"][0])
    assert np.array_equal(out["trip"][0][1].view(np.uint32), np.stack(codes).view(np.uint32))


def test_a_32d_decoder_ignores_the_bits_beyond_its_code(chairs32_decoder):
    dec = chairs32_decoder
    own = E.Engine(dec.layers, dec.latent_in, dec.code_len, device=0)
    o = synth.make_object(X.CHAIRS_SEED, n_surface=100, n_background=30, code_len=32, half=synth.CHAIR_HALF)
    prm = E.gn_params(num_iterations=3)
    code = np.zeros(64, F32)
    code[:32] = _codes([o])[0][:32]
    out = {}
    for tail in (0, 1, None):
        b = own.batch(prm, [o["t_cam_obj_init"]], [o["pts"]], [o["rays"]], [o["depth"]], [code], trace=True)
        if tail is not None:
            live = _random_mask(33)
            live[39:] = tail
            b.set_unknowns(live)
        b.run()
        out[tail] = list(b.results()) + [b.trace(e)[k] for e in range(3) for k in ("H", "b", "dx", "code")]
        b.close()
    lv = _random_mask(33).astype(bool)
    assert out[0][3].tolist() == [0] and _same(out[0], out[1]) and not _same(out[0], out[None])
    dx = out[0][6]
    assert not dx[0][:39][~lv[:39]].any() and not dx[0][39:].any() and np.abs(dx[0][:39][lv[:39]]).max() > 0
    # all of the first 39 live, the tail frozen: no mask at all
    b = own.batch(prm, [o["t_cam_obj_init"]], [o["pts"]], [o["rays"]], [o["depth"]], [code], trace=True)
    live = np.ones(71, np.uint8)
    live[39:] = 0
    b.set_unknowns(live)
    b.run()
    got = list(b.results()) + [b.trace(e)[k] for e in range(3) for k in ("H", "b", "dx", "code")]
    b.close()
    own.close()
    assert _same(got, out[None])


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
def test_a_refused_mask_keeps_the_previous_one(eng, plain):
    o = plain["objs"][0]
    n_it = 2
    b = _joint(eng, [o], E.gn_params(num_iterations=n_it))
    b.set_unknowns(FROZEN["random"])
    want = _run(b, n_it)[0]
    bad = FROZEN["scale"].copy()
    bad[9] = 2
    rc = L.load().dsp_batch_unknowns(b._h, L.ptr(np.ascontiguousarray(bad.reshape(1, 71)), U8P))
    assert rc == -1 and b"neither 0" in L.load().dsp_last_error(eng._h)
    with pytest.raises(L.DspError, match=r"\(-1\)"):
        b.set_unknowns(bad)
    with pytest.raises(ValueError):
        b.set_unknowns(np.ones((2, 71), np.uint8))
    assert _same(want, _run(b, n_it)[0])                     # the previous mask, by bits
    stale = b._h.value
    b.close()
    assert L.load().dsp_batch_unknowns(C.c_void_p(stale), None) == -1 and L.load().dsp_batch_unknowns(C.c_void_p(stale), L.ptr(FROZEN["scale"], U8P)) == -1


def test_an_allocation_failure_leaves_the_mask_off_and_the_batch_running(eng, plain):
    o = plain["objs"][0]
    n_it = 2
    b = _joint(eng, [o], E.gn_params(num_iterations=n_it))
    free = _run(b, n_it)[0]
    live = np.ascontiguousarray(FROZEN["random"].reshape(1, 71))
    eng.trim()
    eng.fail_alloc(0)
    rc = L.load().dsp_batch_unknowns(b._h, L.ptr(live, U8P))
    eng.fail_alloc(-1)
    assert rc == -3 and b"out of device memory" in L.load().dsp_last_error(eng._h)          # DSP_E_NOMEM
    assert _same(free, _run(b, n_it)[0])                     # the mask off, the batch usable
    b.set_unknowns(live)
    got = _run(b, n_it)[0]
    assert got[3].tolist() == [0] and not np.array_equal(got[0], free[0])
    b.close()


# ---- 9. the tool -----------------------------------------------------------------------------------------------------------------------
def test_reoptimise_map_with_the_pose_live_keeps_the_maps_codes(tmp_path, eng):
    from dsp_slam_amd.map_objects import read_map_objects, write_map_objects
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import reoptimise_map as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    map_dir = tmp_path / "map"
    (map_dir / "observations").mkdir(parents=True)
    objs = []
    rng = np.random.default_rng(17)
    for i, (n_s, n_b) in enumerate(((120, 40), (97, 35), (150, 30))):
        o = synth.make_object(7100 + i, n_surface=n_s, n_background=n_b)
        objs.append(dict(id=5 * i + 2, pose=o["t_cam_obj_init"].astype(np.float64), code=(0.05 * rng.standard_normal(64)).astype(np.float32)))
        if i != 1:                      # object 7 has no observation
            np.savez(map_dir / "observations" / ("%d.npz" % (5 * i + 2)), pts=o["pts"], rays=o["rays"], depth=o["depth"], t_world_cam=np.eye(4))
    write_map_objects(str(map_dir / "MapObjects.txt"), objs)
    objs = read_map_objects(str(map_dir / "MapObjects.txt"))
    obs = tool.load_observations(str(map_dir), objs)
    prm = E.gn_params(num_iterations=3)
    free, _ = tool.reoptimise([eng], prm, objs, obs, 64)
    out, st = tool.reoptimise([eng], prm, objs, obs, 64, unknowns=["pose"])
    assert st["n_good"] == 2
    for a, f, m in zip(out, free, objs):
        assert np.array_equal(np.asarray(a["code"], F32).view(np.uint32), np.asarray(m["code"], F32).view(np.uint32))          # the map's codes, bit for bit
    assert not np.array_equal(out[0]["pose"], objs[0]["pose"]) and not np.array_equal(free[0]["code"], objs[0]["code"])
    with pytest.raises(ValueError):
        tool.reoptimise([eng], prm, objs, obs, 64, unknowns=["poze"])
    # the command-line flag
    import json
    import runpy
    from dsp_slam_amd import fixtures
    from dsp_slam_amd.map_objects import read_map_objects as read
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    cfg["DeepSDF_DIR"] = fixtures.materialize_decoder_dir("cars", str(tmp_path / "cars_64"))
    cfg.setdefault("data_type", "KITTI")
    with open(str(tmp_path / "cfg.json"), "w") as f:
        json.dump(cfg, f)
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    old_argv = sys.argv
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    sys.path.insert(0, pkg)
    sys.argv = ["reoptimise_map.py", "--config", str(tmp_path / "cfg.json"), "--map_dir", str(map_dir), "--gpus", "1", "--unknowns", "pose", "--out", str(tmp_path / "cli.txt")]
    try:
        runpy.run_path(os.path.join(ROOT, "tools", "reoptimise_map.py"), run_name="__main__")
    finally:
        sys.argv = old_argv
        sys.path.remove(pkg)
        for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
            del sys.modules[m]
    cli = read(str(tmp_path / "cli.txt"))
    for a, m in zip(cli, objs):
        assert np.array_equal(np.asarray(a["code"], F32).view(np.uint32), np.asarray(m["code"], F32).view(np.uint32))
    assert not np.array_equal(cli[0]["pose"], objs[0]["pose"])


def test_worst_figures_are_printed():
    """(runs last in this file) The worst figures tests 4, 5 and 7 measured, for profiles/unknowns.md."""
    print("worst figures: %s" % {k: "%.3e" % v for k, v in sorted(WORST.items())})
    parity_log(kind="unknowns_worst", **WORST)
