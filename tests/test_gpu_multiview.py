"""GPU: multi-view reconstruction (dsp_reconstruct_multiview / dsp_batch_create_multiview) -- one pose and one code per object, many cameras.

  * one view per object IS dsp_reconstruct_batch: bit for bit, detection-size and cfg2-size objects, prepass on and off;
  * a ragged batch of 1-, 2- and 4-view objects equals each object run alone, bit for bit, in any object order, run after run;
  * the device at the REFERENCE'S recorded states (tests/golden/golden_multiview_cars3.npz): state and per-view depths injected, one iteration:
    per-view V, K and checksums identical, pooled H, b, loss within 1e-4 (the comparison of tests/test_gpu_forensics.py);
  * a view that joins late follows the oracle's per-iteration V and K; three one-sided views beat the best single view; the launch forms
    forced on a group with an empty view give the automatic plan's bits;
  * every iteration of a three-view run, linearised by the composed oracle (tests/multiview_oracle.py) at the device's own state: per-view
    sample sets identical, pooled H / b / loss within the bounds the single-view tests use (1e-4);
  * one observation dealt into two views of one camera: same sets, H / b up to fp32 summation order (4 x the oracle's own difference);
  * no view with 10 samples -> FEW_SAMPLES; a view that has none contributes no render rows; a NaN depth in one view fails that object
    alone; refused arguments; a forced prepass margin of 2e-5 trips the guard and the whole group returns its prepass-off bits.
"""
import json

import numpy as np
import pytest

import multiview_oracle as MV
from oracle import dsp_oracle as O
from dsp_slam_amd import _lib as L, engine as E, synth
from conftest import golden

pytestmark = pytest.mark.gpu
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def one_view(o):
    return [dict(t_ref_cam=EYE, pts=o["pts"], rays=o["rays"], depth=o["depth"])]


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("size", ["detection", "cfg2"])
@pytest.mark.parametrize("prepass", [-1, 0])
def test_one_view_is_reconstruct_batch(eng, size, prepass):
    objs = [synth.make_object(40 + i, n_surface=120, n_background=30) for i in range(3)] if size == "detection" else [synth.make_object(11, n_surface=2000, n_background=500)]
    prm = E.gn_params(num_iterations=4)
    out = {}
    for kind in ("single", "multi"):
        if kind == "single":
            b = eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs])
        else:
            b = eng.multiview_batch(prm, [o["t_cam_obj_init"] for o in objs], [one_view(o) for o in objs])
        b.set_prepass(prepass)
        b.run()
        out[kind] = b.results()
        b.close()
    assert (out["single"][3] == 0).all()
    assert same_bits(out["single"], out["multi"])
    # and the one-shot entry point
    if prepass == -1:
        assert same_bits(out["single"], eng.reconstruct_multiview_batch(prm, [o["t_cam_obj_init"] for o in objs], [one_view(o) for o in objs]))


def _mv_objects():
    return [synth.make_object_multiview(20 + i, n_views=nv, n_surface=150, n_background=40) for i, nv in enumerate([1, 2, 4, 2])]


def test_ragged_batch_equals_each_object_alone_in_any_order(eng):
    objs = _mv_objects()
    prm = E.gn_params(num_iterations=4)
    alone = [eng.reconstruct_multiview_batch(prm, [o["t_cam_obj_init"]], [o["views"]]) for o in objs]
    assert all(a[3][0] == 0 for a in alone)
    for order in ([0, 1, 2, 3], [2, 0, 3, 1], [3, 2, 1, 0]):
        r1 = eng.reconstruct_multiview_batch(prm, [objs[i]["t_cam_obj_init"] for i in order], [objs[i]["views"] for i in order])
        r2 = eng.reconstruct_multiview_batch(prm, [objs[i]["t_cam_obj_init"] for i in order], [objs[i]["views"] for i in order])
        assert same_bits(r1, r2), "two runs of the same batch differ"
        for k, i in enumerate(order):
            assert same_bits([x[k] for x in r1], [x[0] for x in alone[i]]), "object %d in order %s differs from its run alone" % (i, order)
    # a two-view object is not its reference view alone: the second view is used
    ref_only = eng.reconstruct_multiview_batch(prm, [objs[1]["t_cam_obj_init"]], [objs[1]["views"][:1]])
    assert not np.array_equal(ref_only[1], alone[1][1])


def test_every_iteration_against_the_composed_oracle(eng, oracle_decoder):
    """The device's pooled system of every iteration against the composed oracle restarted from the device's own state and per-view depths."""
    o = synth.make_object_multiview(31, n_views=3, n_surface=300, n_background=80)
    n_it = 4
    b = eng.multiview_batch(E.gn_params(num_iterations=n_it), [o["t_cam_obj_init"]], [o["views"]], trace=True)
    b.run()
    assert b.results()[3][0] == 0
    o1 = O.GNParams(num_iterations=1)
    for e in range(n_it):
        tr, tv = b.trace(e), b.trace_views(e)
        otr = []
        MV.reconstruct_object_multiview(oracle_decoder, o1, None, o["views"], tr["code"][0], trace=otr, t_obj_cam0=tr["t_obj_cam"][0], depths_override=tv["depths"])
        ov = otr[0]["views"]
        print("iteration %d: V %s / %s, K %s / %s" % (e, tv["V"].tolist(), [v["V"] for v in ov], tv["K"].tolist(), [v["K"] for v in ov]))
        for k, v in enumerate(ov):
            assert (int(tv["V"][k]), int(tv["K"][k])) == (v["V"], v["K"])
            assert (int(tv["set_sums"][k][0]), int(tv["set_sums"][k][1])) == (v["vsum"], v["ksum"]), "view %d: sample sets differ" % k
            assert np.array_equal(tv["t_obj_cam"][k], v["t_obj_cam"])
        assert int(tr["V"][0]) == sum(v["V"] for v in ov) and int(tr["K"][0]) == otr[0]["K"]
        eh = np.abs(tr["H"][0] - otr[0]["H"]).max() / np.abs(otr[0]["H"]).max()
        eb = np.abs(tr["b"][0] - otr[0]["b"]).max() / np.abs(otr[0]["b"]).max()
        print("iteration %d: rel dH %.3e, rel db %.3e" % (e, eh, eb))
        if e == n_it - 1:       # the result's loss is the loss at the last linearisation point (optimizer.py:155,200-203)
            assert abs(float(b.results()[2][0]) - otr[0]["loss"]) <= 1e-4 * abs(otr[0]["loss"])
        # the single-view tests' comparison (tests/test_gpu_forensics.py): 1e-4 on H and the loss, 1e-4 of b's largest entry on b, where
        # b[3:6] also carries the rotation prior's residual, quantised to ulp(1) in front of the factor k4 = 1e7 (_rot_prior_bound)
        tol_b = np.full(71, 1e-4 * np.abs(otr[0]["b"]).max())
        tol_b[3:6] += MV.rot_prior_bound(otr[0]["H"], 1e7)
        assert eh < 1e-4 and np.all(np.abs(tr["b"][0] - otr[0]["b"]) <= tol_b), (e, eh, eb)
    b.close()


def test_split_into_two_views_of_one_camera(eng, oracle_decoder):
    o = synth.make_object(5, n_surface=160, n_background=40)
    whole, split = [], []
    o1 = O.GNParams(num_iterations=1)
    MV.reconstruct_object_multiview(oracle_decoder, o1, o["t_cam_obj_init"], one_view(o), trace=whole)
    MV.reconstruct_object_multiview(oracle_decoder, o1, o["t_cam_obj_init"], MV.split_views(o), trace=split)
    oh = np.abs(whole[0]["H"] - split[0]["H"]).max() / np.abs(whole[0]["H"]).max()
    ob = np.abs(whole[0]["b"] - split[0]["b"]).max() / np.abs(whole[0]["b"]).max()
    prm = E.gn_params(num_iterations=1)
    tr = []
    for views in (one_view(o), MV.split_views(o)):
        b = eng.multiview_batch(prm, [o["t_cam_obj_init"]], [views], trace=True)
        b.run()
        tr.append(b.trace(0))
        b.close()
    a, s = tr
    assert int(a["V"][0]) == int(s["V"][0]) and int(a["K"][0]) == int(s["K"][0])
    dh = np.abs(a["H"][0] - s["H"][0]).max() / np.abs(a["H"][0]).max()
    db = np.abs(a["b"][0] - s["b"][0]).max() / np.abs(a["b"][0]).max()
    print("split vs unsplit: oracle rel dH %.3e db %.3e; device rel dH %.3e db %.3e" % (oh, ob, dh, db))
    assert dh <= 4 * oh and db <= 4 * ob


def _away_view(o, n_pts=50):
    return dict(t_ref_cam=EYE, pts=o["pts"][:n_pts], rays=np.tile(np.array([[5.0, 5.0, 1.0]], np.float32), (30, 1)), depth=np.zeros(0, np.float32))


def test_views_without_samples_and_failures_stay_local(eng, oracle_decoder):
    objs = [synth.make_object(60 + i, n_surface=150, n_background=40) for i in range(3)]
    prm = E.gn_params(num_iterations=3)
    t0 = [o["t_cam_obj_init"] for o in objs]
    base = eng.reconstruct_multiview_batch(prm, t0, [one_view(o) for o in objs])
    assert (base[3] == 0).all()
    # every view of object 1 misses the object: FEW_SAMPLES, its neighbours keep their bits
    views = [one_view(objs[0]), [_away_view(objs[1]), _away_view(objs[1])], one_view(objs[2])]
    r = eng.reconstruct_multiview_batch(prm, t0, views)
    assert r[3].tolist() == [0, L.OBJ_FEW_SAMPLES, 0]
    assert same_bits([x[[0, 2]] for x in r], [x[[0, 2]] for x in base])
    # a view without in-sphere samples beside a good one: no render rows from it, its surface points count (the composed oracle agrees)
    views[1] = one_view(objs[1]) + [_away_view(objs[1])]
    b = eng.multiview_batch(prm, t0, views, trace=True)
    b.run()
    r = b.results()
    assert r[3].tolist() == [0, 0, 0]
    tv, tr = b.trace_views(0), b.trace(0)
    assert int(tv["V"][2]) < 10 and int(tv["K"][2]) == 0
    otr = []
    MV.reconstruct_object_multiview(oracle_decoder, O.GNParams(num_iterations=1), None, views[1], tr["code"][1], trace=otr, t_obj_cam0=tr["t_obj_cam"][1],
                                    depths_override=tv["depths"][1:3])
    assert otr[0]["views"][1]["none"] and int(tr["K"][1]) == otr[0]["K"]
    assert np.abs(tr["H"][1] - otr[0]["H"]).max() / np.abs(otr[0]["H"]).max() < 1e-4
    b.close()
    # a NaN depth in ONE view of object 1 fails that object alone
    bad = dict(views[1][0], depth=views[1][0]["depth"].copy())
    bad["depth"][3] = np.nan
    r = eng.reconstruct_multiview_batch(prm, t0, [one_view(objs[0]), [bad, _away_view(objs[1])], one_view(objs[2])])
    assert r[3].tolist() == [0, L.OBJ_NAN, 0]
    assert same_bits([x[[0, 2]] for x in r], [x[[0, 2]] for x in base])


def test_refused_arguments(eng):
    o = synth.make_object_multiview(3, n_views=2, n_surface=60, n_background=20)
    prm = E.gn_params(num_iterations=1)
    ok = eng.reconstruct_multiview_batch(prm, [o["t_cam_obj_init"]], [o["views"]])
    assert ok[3][0] == 0

    def refused(views_per_object, t=None):
        with pytest.raises(L.DspError):
            eng.reconstruct_multiview_batch(prm, t or [o["t_cam_obj_init"]] * len(views_per_object), views_per_object)

    refused([o["views"], []])                                             # an object without views (view_off not increasing)
    shear = o["views"][1]["t_ref_cam"].copy()
    shear[0, 1] += 1e-3
    refused([[o["views"][0], dict(o["views"][1], t_ref_cam=shear)]])      # not rigid: R^T R - I
    row = o["views"][1]["t_ref_cam"].copy()
    row[3, 0] = 1e-3
    refused([[o["views"][0], dict(o["views"][1], t_ref_cam=row)]])        # not rigid: the bottom row
    refused([[o["views"][1], o["views"][0]]])                             # view 0 is not the identity
    b = eng.multiview_batch(prm, [o["t_cam_obj_init"]], [o["views"]])
    with pytest.raises(L.DspError):
        b.set_compute(L.COMPUTE_F16)                                      # the low-precision compute mode does not take groups
    b.close()


def test_guard_trip_reruns_the_whole_group(eng):
    objs = [synth.make_object_multiview(70 + i, n_views=2, n_surface=150, n_background=40) for i in range(2)]
    prm = E.gn_params(num_iterations=3)
    args = ([o["t_cam_obj_init"] for o in objs], [o["views"] for o in objs])
    b = eng.multiview_batch(prm, *args)
    b.set_prepass(0)
    b.run()
    off = b.results()
    b.set_prepass(L.PREPASS_F16, 2e-5)        # a margin below the prepass kernel's error: the guard must trip
    b.run()
    st = b.stats()
    got = b.results()
    b.close()
    eng.prepass_reset_guard()
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_trips"] > 0
    assert same_bits(off, got)


def test_linearisation_at_the_reference_recorded_states(eng):
    g = golden("golden_multiview_cars3.npz")
    cfg = json.loads(str(g["cfg_json"]))
    prm = E.params_from_configs(cfg)
    k4 = cfg["optimizer"]["joint_optim"]["k4"]
    views = MV.golden_views(g)
    b = eng.multiview_batch(prm, [g["in_t_cam_obj_init"]], [views], trace=True)
    b.set_iterations(1)
    mask = np.ones(71, bool)
    mask[3:6] = False
    for e in range(g["it_H"].shape[0]):
        b.set_start_state([g["it_t_obj_cam"][e]], [g["it_code"][e]], g["it_depths"][e])
        b.run()
        t, code, loss, status = b.results()
        assert status[0] == 0
        tr, tv = b.trace(0), b.trace_views(0)
        assert np.array_equal(tr["t_obj_cam"][0], g["it_t_obj_cam"][e]) and np.array_equal(tr["code"][0], g["it_code"][e])
        assert np.array_equal(tv["depths"][:, :50], g["it_depths"][e]) and np.array_equal(tv["t_obj_cam"], g["it_t_views"][e])
        print("iteration %d: V %s K %s" % (e, tv["V"].tolist(), tv["K"].tolist()))
        assert tv["V"].tolist() == g["it_V"][e].tolist() and tv["K"].tolist() == g["it_K"][e].tolist()
        assert tv["set_sums"][:, 0].astype(np.int64).tolist() == g["it_vsum"][e].tolist() and tv["set_sums"][:, 1].astype(np.int64).tolist() == g["it_ksum"][e].tolist()
        h_ref, b_ref = g["it_H"][e], g["it_b"][e]
        rh = np.abs(tr["H"][0] - h_ref).max() / np.abs(h_ref).max()
        rb = np.abs(tr["b"][0][mask] - b_ref[mask]).max() / np.abs(b_ref).max()
        rl = abs(float(loss[0]) - float(g["it_loss"][e])) / abs(float(g["it_loss"][e]))
        print("iteration %d: rel dH %.3e, rel db %.3e, rel dloss %.3e" % (e, rh, rb, rl))
        assert rh < 1e-4 and rb < 1e-4 and rl <= 1e-4
        assert np.all(np.abs(tr["b"][0][3:6] - b_ref[3:6]) <= MV.rot_prior_bound(h_ref, k4) + 1e-4 * np.abs(b_ref).max())
    b.close()


def test_a_view_that_joins_late(eng, oracle_decoder):
    t, views = MV.late_join_case()
    n_it = 4
    otr = []
    ores = MV.reconstruct_object_multiview(oracle_decoder, O.GNParams(num_iterations=n_it), t, views, trace=otr)
    ovk = [[(v["V"], v["K"]) for v in i["views"]] for i in otr]
    assert ores["is_good"] and ovk[0][1][0] < 10 and any(vk[1][0] >= 10 and vk[1][1] > 0 for vk in ovk[1:])
    for forms in (None, dict(set_wave_bookkeeping=0, set_prepass=0), dict(set_wave_bookkeeping=1, set_speculative_band=1)):
        b = eng.multiview_batch(E.gn_params(num_iterations=n_it), [t], [views], trace=True)
        for k, v in (forms or {}).items():
            getattr(b, k)(v)
        b.run()
        assert b.results()[3][0] == 0
        dvk = []
        for e in range(n_it):
            tv = b.trace_views(e)
            dvk.append([(int(tv["V"][k]), int(tv["K"][k])) for k in range(2)])
        b.close()
        print("forms %s: late view (V, K) device %s oracle %s" % (forms, [x[1] for x in dvk], [x[1] for x in ovk]))
        assert dvk == ovk


def test_three_one_sided_views_beat_the_best_single_view(eng):
    o, starts = MV.one_sided_case()
    prm = E.gn_params(num_iterations=6)
    r3 = eng.reconstruct_multiview_batch(prm, [o["t_cam_obj_init"]], [o["views"]])
    r1 = eng.reconstruct_batch(prm, starts, [v["pts"] for v in o["views"]], [v["rays"] for v in o["views"]], [v["depth"] for v in o["views"]])
    assert r3[3][0] == 0 and (r1[3] == 0).all()
    e3, e1 = MV.code_error(r3[1][0], o), [MV.code_error(c, o) for c in r1[1]]
    print("code error: three views %.4f, single views %s" % (e3, e1))
    assert e3 < min(e1)


FORMS = [dict(set_wave_bookkeeping=1), dict(set_wave_bookkeeping=0), dict(set_tail_split=1, set_wave_bookkeeping=0), dict(set_cluster_tiles=1),
         dict(set_speculative_band=1, set_wave_bookkeeping=1), dict(set_speculative_band=0), dict(set_split_rows=0, set_mask_reuse=1),
         dict(set_mixed_reuse=1), dict(set_prepass=0)]


@pytest.mark.parametrize("forms", FORMS, ids=lambda f: "+".join("%s=%s" % kv for kv in f.items()))
def test_launch_forms_on_a_group_with_an_empty_view(eng, forms):
    o = synth.make_object(64, n_surface=150, n_background=40)
    views = [one_view(o) + [_away_view(o)], [_away_view(o), _away_view(o)]]
    t0 = [o["t_cam_obj_init"]] * 2
    prm = E.gn_params(num_iterations=3)
    auto = eng.reconstruct_multiview_batch(prm, t0, views)
    assert auto[3].tolist() == [0, L.OBJ_FEW_SAMPLES]
    b = eng.multiview_batch(prm, t0, views)
    for k, v in forms.items():
        getattr(b, k)(v)
    b.run()
    got = b.results()
    b.close()
    assert same_bits(auto, got)
