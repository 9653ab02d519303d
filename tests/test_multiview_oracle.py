"""CPU: the composed multi-view oracle (tests/multiview_oracle.py) and the host-side surface of multi-view reconstruction.

  * one view: the composition IS oracle.dsp_oracle.reconstruct_object -- same H, b, dx, result, bit for bit;
  * one observation dealt alternately into two views of the same camera: the same sample sets, and H, b up to fp32 summation order;
  * the reference pin: every recorded iteration of tests/golden/golden_multiview_cars3.npz (tools/make_golden_multiview.py: the unmodified
    reference's own terms per view, pooled) is reproduced by the composition at the recorded state -- sets identical, H to 1e-4 relative,
    b to 1e-4 of its largest entry (the bounds of tests/test_oracle_golden.py);
  * a view that joins late, and three one-sided views against the best single view, on inputs chosen here for the GPU tests;
  * the library declares, exports and binds the multi-view entry points; synth.make_object_multiview draws rigid view transforms.
"""
import numpy as np

import json

import multiview_oracle as MV
from conftest import golden
from oracle import dsp_oracle as O
from dsp_slam_amd import _lib as L, synth

PRM = dict(k1=1.0, k2=100.0, k3=0.25, k4=1e7, b1=0.2, b2=0.025, lr=1.0, s_damp=1.0, num_iterations=2, num_depth_samples=50, cut_off=0.01)
EYE = np.eye(4, dtype=np.float32)


def _small(seed=3, n=160, nb=40):
    return synth.make_object(seed, n_surface=n, n_background=nb)


def test_one_view_is_the_single_view_oracle(oracle_decoder):
    o = _small()
    prm = O.GNParams(**PRM)
    tr1, trm = [], []
    ref = O.reconstruct_object(oracle_decoder, prm, o["t_cam_obj_init"], o["pts"], o["rays"], o["depth"], trace=tr1)
    got = MV.reconstruct_object_multiview(oracle_decoder, prm, o["t_cam_obj_init"], [dict(t_ref_cam=EYE, pts=o["pts"], rays=o["rays"], depth=o["depth"])],
                                          trace=trm)
    assert ref["is_good"] and got["is_good"]
    for a, b in zip(tr1, trm):
        assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["b"], b["b"]) and np.array_equal(a["dx"], b["dx"])
        assert (a["V"], a["K"], a["vsum"], a["ksum"]) == tuple(b["views"][0][k] for k in ("V", "K", "vsum", "ksum"))
    assert np.array_equal(ref["t_cam_obj"], got["t_cam_obj"]) and np.array_equal(ref["code"], got["code"]) and ref["loss"] == got["loss"]


def test_split_into_two_views_of_one_camera(oracle_decoder):
    o = _small(5)
    prm = O.GNParams(**dict(PRM, num_iterations=1))
    whole, split = [], []
    MV.reconstruct_object_multiview(oracle_decoder, prm, o["t_cam_obj_init"], [dict(t_ref_cam=EYE, pts=o["pts"], rays=o["rays"], depth=o["depth"])], trace=whole)
    MV.reconstruct_object_multiview(oracle_decoder, prm, o["t_cam_obj_init"], MV.split_views(o), trace=split)
    a, b = whole[0], split[0]
    assert a["M"] == b["M"] and a["K"] == b["K"] and a["views"][0]["V"] == sum(v["V"] for v in b["views"])
    # fp32 Gram sums of ~200 rows in two orders: a few ulp of the largest partial sums
    dh = np.abs(a["H"] - b["H"]).max() / np.abs(a["H"]).max()
    db = np.abs(a["b"] - b["b"]).max() / np.abs(a["b"]).max()
    print("split vs unsplit (composed oracle): rel dH %.3e, rel db %.3e" % (dh, db))
    assert dh < 200 * 2.0 ** -24 and db < 200 * 2.0 ** -24


def test_a_view_without_samples_contributes_no_render_rows(oracle_decoder):
    o = _small(7)
    prm = O.GNParams(**dict(PRM, num_iterations=1))
    away = dict(t_ref_cam=EYE, pts=o["pts"][:50], rays=np.tile(np.array([[5.0, 5.0, 1.0]], np.float32), (30, 1)), depth=np.zeros(0, np.float32))
    tr = []
    r = MV.reconstruct_object_multiview(oracle_decoder, prm, o["t_cam_obj_init"], [dict(t_ref_cam=EYE, pts=o["pts"], rays=o["rays"], depth=o["depth"]), away], trace=tr)
    assert r["is_good"] and tr[0]["views"][1]["none"] and tr[0]["views"][1]["K"] == 0 and tr[0]["M"] == o["pts"].shape[0] + 50
    assert tr[0]["K"] == tr[0]["views"][0]["K"]
    r = MV.reconstruct_object_multiview(oracle_decoder, prm, o["t_cam_obj_init"], [away, away])
    assert not r["is_good"] and r["status"] == 1


def test_library_binds_the_multiview_entry_points():
    lib = L.load()
    for name in ("dsp_reconstruct_multiview", "dsp_batch_create_multiview", "dsp_batch_trace_views"):
        assert hasattr(lib, name) and name in {n for n, _, _ in L.SYMBOLS}
    assert lib.dsp_abi_version() == 6


def test_synthetic_views_are_rigid_and_consistent():
    o = synth.make_object_multiview(1, n_views=3, n_surface=50, n_background=10)
    assert len(o["views"]) == 3 and np.array_equal(o["views"][0]["t_ref_cam"], EYE)
    s = float(o["scale"])
    for v in o["views"]:
        t = v["t_ref_cam"].astype(np.float64)
        assert np.abs(t[:3, :3].T @ t[:3, :3] - np.eye(3)).max() < 1e-5 and np.array_equal(t[3], [0, 0, 0, 1])
        # the view's points, moved to the reference camera and into the object frame, lie on the generating surface
        p_ref = v["pts"].astype(np.float64) @ t[:3, :3].T + t[:3, 3]
        t_oc = np.linalg.inv(o["t_cam_obj_gt"].astype(np.float64))
        p_o = p_ref @ t_oc[:3, :3].T + t_oc[:3, 3]
        assert np.abs(synth.rounded_box_sdf(p_o, o["code_gt"][:3].astype(np.float64))).max() < 1e-4 * s
        assert v["rays"].shape[0] == 60 and v["depth"].shape[0] == 50


def test_composition_reproduces_the_reference_recording(oracle_decoder):
    g = golden("golden_multiview_cars3.npz")
    prm = O.GNParams.from_configs(json.loads(str(g["cfg_json"])))
    prm.num_iterations = 1
    views = MV.golden_views(g)
    assert len(views) == 3
    mask = np.ones(71, bool)
    mask[3:6] = False
    for e in range(g["it_H"].shape[0]):
        # the depth samples the composition derives from T_oc_v are the reference's up to the 1-2 ulp by which numpy's and torch's fp32
        # inverse / pow differ (the single-view goldens: dsp_batch_debug_start_state in include/dsp_gn.h); the linearisation then runs on the
        # recorded samples, as tests/test_oracle_golden.py runs the single-view oracle on them
        for v, view in enumerate(views):
            d = MV.view_state(g["it_t_obj_cam"][e], view["t_ref_cam"], prm.num_depth_samples)[1]
            assert np.abs(d - g["it_depths"][e][v]).max() <= 4 * 2.0 ** -24 * np.abs(d).max()
        tr = []
        MV.reconstruct_object_multiview(oracle_decoder, prm, None, views, g["it_code"][e], trace=tr, t_obj_cam0=g["it_t_obj_cam"][e],
                                        depths_override=g["it_depths"][e])
        it = tr[0]
        for v, pv in enumerate(it["views"]):
            assert np.array_equal(pv["t_obj_cam"], g["it_t_views"][e][v])
            assert (pv["V"], pv["K"], pv["vsum"], pv["ksum"]) == tuple(int(g["it_" + k][e][v]) for k in ("V", "K", "vsum", "ksum"))
        assert np.abs(it["H"] - g["it_H"][e]).max() / np.abs(g["it_H"][e]).max() < 1e-4
        bmax = np.abs(g["it_b"][e]).max()
        assert np.abs(it["b"][mask] - g["it_b"][e][mask]).max() < 1e-4 * bmax
        assert np.all(np.abs(it["b"][3:6] - g["it_b"][e][3:6]) <= MV.rot_prior_bound(g["it_H"][e], prm.k4) + 1e-4 * bmax)
        assert abs(it["loss"] - float(g["it_loss"][e])) <= 1e-4 * abs(float(g["it_loss"][e]))


def test_a_view_that_joins_late(oracle_decoder):
    t, views = MV.late_join_case()
    tr = []
    r = MV.reconstruct_object_multiview(oracle_decoder, O.GNParams(**dict(PRM, num_iterations=4)), t, views, trace=tr)
    vk = [(i["views"][1]["V"], i["views"][1]["K"]) for i in tr]
    print("late view (V, K) per iteration:", vk)
    assert r["is_good"] and vk[0][0] < 10 and tr[0]["views"][1]["none"] and any(v >= 10 and k > 0 for v, k in vk[1:])


def test_three_one_sided_views_beat_the_best_single_view(oracle_decoder):
    o, starts = MV.one_sided_case()
    prm = O.GNParams(**dict(PRM, num_iterations=6))
    r3 = MV.reconstruct_object_multiview(oracle_decoder, prm, o["t_cam_obj_init"], o["views"])
    singles = [MV.reconstruct_object_multiview(oracle_decoder, prm, s, [dict(v, t_ref_cam=EYE)]) for v, s in zip(o["views"], starts)]
    assert r3["is_good"] and all(r["is_good"] for r in singles)
    e3, e1 = MV.code_error(r3["code"], o), [MV.code_error(r["code"], o) for r in singles]
    print("code error: three views %.4f, single views %s" % (e3, e1))
    assert e3 < min(e1)
