"""The launch forms a test can pin, in one table: for every named form the Batch.set_* pins, the LaunchPlan fields (csrc/launch_plan.h)
those pins must produce, and what the run's stats() must show -- and the batches the feature tests run them on (SHAPES), so that
tests/test_feature_forms_plan.py (CPU) can show that every form reaches the plan it names on exactly the shapes
tests/test_gpu_feature_forms.py (GPU) runs.  The plan of a row of inputs comes from the library's host hook, as in tests/test_launch_plan.py.
Test helper, not a test."""
import numpy as np

from dsp_slam_amd import _lib as L
from test_launch_plan import INPUTS, PLAN, base_row, evaluate

N_CU, N_CLUSTERS = 256, 64        # an MI355X

# setter (Batch.set_<name>) -> (the plan input it writes, its "automatic" value)
SETTERS = {"wave_bookkeeping": ("fused_bookkeeping", -1), "split_rows": ("split_rows", -1), "mask_reuse": ("mask_reuse", -1), "mixed_reuse": ("mixed_reuse", -1),
           "speculative_band": ("speculative", -1), "tail_split": ("tail_split", -1), "cluster_tiles": ("cluster_tiles", -1), "direct_tiles": ("direct_tiles", -1),
           "prepass": ("prepass", -1), "prepass_tile": ("lp_tile", -1), "kernel_timing": ("kernel_timing", -1), "ray_passes": ("n_ray_passes", 0),
           "compute": ("compute", 0), "lp_small_batches": ("lp_small", -1)}


def _form(pins, plan, one_object=False, pose_ok=False):
    return dict(pins=pins, plan=plan, one_object=one_object, pose_ok=pose_ok)


# name -> pins {setter: value}, plan {field: value} the pins must produce on every shape the form runs on; one_object: only on one-object
# batches (that are not multi-view); pose_ok: a form a pose-only batch has too.  The pins are those of the FORMS tables of
# tests/test_gpu_multiview.py, test_gpu_early_stop.py and test_gpu_mono_shape.py, completed where a pin alone does not reach its form on a
# small batch: tail tiles need the forward launch out of the latency form, the mixed form needs the latency form without the speculative band,
# and the cluster form needs the mixed form off where the expected list is too long for the plan to prefer it (the cluster kernel then looks at
# the real tile count and hands lists of more than cluster_max_tiles tiles to the latency-form kernel behind it).
FORMS = {
    "wave": _form(dict(wave_bookkeeping=1), dict(bookkeeping_form=2)),
    "block": _form(dict(wave_bookkeeping=0), dict(bookkeeping_form=0, speculative_band=0, direct_tiles=0)),
    "block+tail_split": _form(dict(wave_bookkeeping=0, tail_split=1, split_rows=0, mask_reuse=0),
                              dict(bookkeeping_form=0, tail_split=1, split_fwd=0, split_rows=0, reuse_throughput=0, jac_tile_pts=64, fwd_tile_pts=64)),
    "cluster_on": _form(dict(cluster_tiles=1, split_rows=1, mixed_reuse=0), dict(cluster=1, split_rows=1, mixed_reuse=0, jac_tile_pts=16), pose_ok=True),
    "cluster_off": _form(dict(cluster_tiles=0, split_rows=1), dict(cluster=0, split_rows=1, jac_tile_pts=16), pose_ok=True),
    "split_rows": _form(dict(split_rows=1, mask_reuse=0), dict(split_rows=1, mask_reuse=0, jac_tile_pts=16), pose_ok=True),
    "split_rows_off": _form(dict(split_rows=0), dict(split_rows=0, split_fwd=0, cluster=0, jac_tile_pts=64, fwd_tile_pts=64), pose_ok=True),
    "speculative_on": _form(dict(speculative_band=1, wave_bookkeeping=1), dict(speculative_band=1, bookkeeping_form=2, mixed_reuse=0)),
    "speculative_off": _form(dict(speculative_band=0), dict(speculative_band=0)),
    "mixed_reuse": _form(dict(mixed_reuse=1, split_rows=1, speculative_band=0), dict(mixed_reuse=1, mask_reuse=1, split_rows=1, speculative_band=0, cluster=0,
                                                                                       reuse_throughput=0)),
    "throughput": _form(dict(split_rows=0, mask_reuse=1, wave_bookkeeping=0),
                        dict(reuse_throughput=1, mask_reuse=1, bookkeeping_form=0, jac_tile_pts=64, fwd_tile_pts=64, split_rows=0, split_fwd=0, tail_split=0, cluster=0,
                             mixed_reuse=0, speculative_band=0, direct_tiles=0)),
    "mask_reuse_off": _form(dict(mask_reuse=0), dict(mask_reuse=0, mixed_reuse=0, reuse_throughput=0)),
    "prepass_off": _form(dict(prepass=L.PREPASS_OFF), dict(prepass_mode=0, guard_on=0, speculative_band=0, whole=0, fixed_passes=0, hint_passes=2)),
    "prepass_off_one_pass": _form(dict(prepass=L.PREPASS_OFF, ray_passes=1), dict(prepass_mode=0, speculative_band=0, whole=0, fixed_passes=1, hint_passes=0)),
    "prepass_bf16": _form(dict(prepass=L.PREPASS_BF16), dict(prepass_mode=2, guard_on=1)),
    "fixed_10_passes": _form(dict(ray_passes=10), dict(fixed_passes=10, hint_passes=0, whole=0, prepass_mode=1)),
    "prepass_tile_64": _form(dict(prepass_tile=64), dict(lp_tile_pts=64, prepass_mode=1)),
    "prepass_tile_128": _form(dict(prepass_tile=128), dict(lp_tile_pts=128, prepass_mode=1)),
    "direct_tiles_on": _form(dict(direct_tiles=1), dict(direct_tiles=1, bookkeeping_form=2), one_object=True),
    "direct_tiles_off": _form(dict(direct_tiles=0), dict(direct_tiles=0, bookkeeping_form=2), one_object=True),
    "kernel_timing_on": _form(dict(kernel_timing=1), dict(kernel_timing=1)),
}


def forms_for(shape):
    """The names of the forms that apply to a shape, in the table's order."""
    if shape["pose_only"]:
        return [n for n, f in FORMS.items() if f["pose_ok"]]          # all a pose-only plan has: the jacobian launch's form
    one = shape["B"] == 1 and not shape["grouped"]
    return [n for n, f in FORMS.items() if one or not f["one_object"]]


# ---- the shapes --------------------------------------------------------------------------------------------------------------------------
def ragged3():
    import test_gpu_weights as TW
    return TW._ragged_objects()


def detection():
    from dsp_slam_amd import synth
    return [synth.make_object(720, n_surface=250, n_background=150, n_foreground=300)]


def hinted3():
    from dsp_slam_amd import synth
    # (the third with a poor initial estimate, like tests/test_gpu_early_stop.py's third cold object: step control rejects trials on it)
    return [synth.make_object(760, n_surface=150, n_background=200), synth.make_object(761, n_surface=150, n_background=200),
            synth.make_object(762, n_surface=150, n_background=200, t_noise=0.6, yaw_noise_deg=15.0)]


def auto_block17():
    from dsp_slam_amd import synth
    return [synth.make_object(770 + i, n_surface=250, n_background=20, n_foreground=40) for i in range(17)]


def metric3():
    import test_gpu_weights as TW
    return TW._metric_objects()


def step6_sizes():
    """(points, rays) of the six-object batch of tests/test_gpu_step_control.py (three cold objects and their warm-started twins)."""
    return [(160, 200)] * 6


VIEWS18_SEEDS = (91, 92, 93, 94, 95, 96)
AWAY = (3, 1)            # (object, view): replaced by a view whose rays all miss the object
ZERO_OBJECT = 4          # every view of this object holds weight 0 (tests/test_gpu_feature_forms.py)


def views18():
    """Six objects of three views each, built as multiview_metric.case_ragged builds its views (100 surface points + 30 background rays per
    view) and cut raggedly: 60 to 100 points and 10 to 50 foreground + 30 background rays per view (n_fg != M, the monocular layout).  One
    view is test_gpu_multiview._away_view.  -> [dict(t, views)]"""
    import multiview_metric as X
    import test_gpu_multiview as TM
    rng = np.random.default_rng(18)
    objs = []
    for i, seed in enumerate(VIEWS18_SEEDS):
        o = X._mv(seed, n_views=3, n_surface=100, n_background=30)
        views = []
        for k, v in enumerate(o["views"]):
            n_p, n_fg = int(rng.integers(60, 101)), int(rng.integers(10, 51))
            if (i, k) == AWAY:
                views.append(TM._away_view(dict(pts=o["views"][0]["pts"])))        # (the reference camera's points: t_ref_cam is the identity)
                continue
            views.append(dict(t_ref_cam=v["t_ref_cam"], pts=v["pts"][:n_p], rays=np.concatenate([v["rays"][:n_fg], v["rays"][100:]]), depth=v["depth"][:n_fg]))
        objs.append(dict(t=o["t"], views=views))
    return objs


def pose_pair_sizes():
    from conftest import golden
    n = golden("golden_pose_only_8it.npz")["pts"].shape[0]
    return [(n, 0), (n, 0)]


def sizes(objs):
    """(points, rays) per member of a list of objects (single-view) or of dict(t, views) objects (multi-view: the members are the views)."""
    if objs and "views" in objs[0]:
        return [(v["pts"].shape[0], v["rays"].shape[0]) for o in objs for v in o["views"]]
    return [(o["pts"].shape[0], o["rays"].shape[0]) for o in objs]


def shape_of(members, n_depth=50, pose_only=False, grouped=False):
    """The plan inputs of a batch of `members` (points, rays): the arithmetic of test_launch_plan.shape for unequal members -- sample slots
    are rounded up to 64 per member (batch_build)."""
    if pose_only:
        return dict(pose_only=1, B=len(members), D=2, sum_pts=sum(p for p, _ in members), sum_rays=0, cap_s=0, grouped=False)
    return dict(pose_only=0, B=len(members), D=n_depth, sum_pts=sum(p for p, _ in members), sum_rays=sum(r for _, r in members),
                cap_s=sum(-(-r * n_depth // 64) * 64 for _, r in members), grouped=grouped)


def shapes():
    """name -> plan inputs of every batch tests/test_gpu_feature_forms.py runs a form on."""
    out = {"ragged3": shape_of(sizes(ragged3())), "ragged3_d64": shape_of(sizes(ragged3()), 64), "detection": shape_of(sizes(detection())),
           "hinted3": shape_of(sizes(hinted3())), "auto_block17": shape_of(sizes(auto_block17())), "metric3": shape_of(sizes(metric3())),
           "step6": shape_of(step6_sizes()), "views18": shape_of(sizes(views18()), grouped=True), "pose_pair": shape_of(pose_pair_sizes(), pose_only=True)}
    return out


# shape -> the forms tests/test_gpu_feature_forms.py pins on it (None: every form that applies); nothing is pinned on auto_block17
USES = {"ragged3": None, "ragged3_d64": ("block", "throughput"), "detection": None, "hinted3": None, "auto_block17": (), "metric3": ("throughput", "block+tail_split"),
        "step6": ("prepass_off", "fixed_10_passes", "block", "throughput"), "views18": None, "pose_pair": None}
F16_FORMS = ("wave", "block")          # the f16 compute mode (compute = 1, lp_small_batches = 1) on ragged3
F16_PINS = dict(compute=L.COMPUTE_F16, lp_small_batches=1)


def uses(name, shape):
    return list(forms_for(shape) if USES[name] is None else USES[name])


def plan_row(shape, pins=None, n_cu=N_CU, n_clusters=N_CLUSTERS):
    """The row of plan inputs (in the order of test_launch_plan.INPUTS) of a batch of `shape` with `pins` {setter: value} set."""
    r = base_row({k: v for k, v in shape.items() if k != "grouped"}, n_cu, n_clusters)
    for name, value in (pins or {}).items():
        key, _ = SETTERS[name]
        r[key] = (2 if value == 1 else value) if name == "wave_bookkeeping" else value
    if shape["grouped"]:
        r["direct_tiles"] = 0          # plan_run: a multi-view batch is never ONE object
    return [r[k] for k in INPUTS]


def plan_of(shape, pins=None, **chip):
    """The LaunchPlan, as a dict, of a batch of `shape` with `pins` set: the library's own make_launch_plan."""
    out = evaluate(np.array([plan_row(shape, pins, **chip)], np.int32))[0]
    return dict(zip(PLAN, out.tolist()))


def plan_of_form(shape, form, extra=None):
    return plan_of(shape, dict(FORMS[form]["pins"], **(extra or {})) if form else extra)


# ---- on a batch ----------------------------------------------------------------------------------------------------------------------------
def pin(b, pins):
    for name, value in pins.items():
        getattr(b, "set_" + name)(value)


def unpin(b, pins):
    for name in pins:
        getattr(b, "set_" + name)(SETTERS[name][1])


def expected_launches(plan, fronts):
    """(fp32 forward, jacobian, prepass) decoder launches of a run of `fronts` iteration fronts (the iterations, and one more for the pass
    at the returned state when the posterior or the report is on) under `plan`, as batch_run_once counts them."""
    if not (plan["fixed_passes"] or plan["hint_passes"]):          # pose-only: no rays
        return 0, fronts, 0
    passes = 1 if plan["whole"] else (plan["fixed_passes"] or plan["hint_passes"])
    if plan["prepass_mode"]:
        fwd = 0 if (plan["speculative_band"] or plan["lp_compute"]) else 1
        return fronts * fwd, fronts * (1 + plan["reuse_throughput"]), fronts * passes
    return fronts * passes, fronts * (1 + plan["reuse_throughput"]), 0


def check_stats(name, plan, st, fronts, rows_expected=True, must_cluster=False):
    """What stats() shows of the form that ran.  rows_expected: the run kept render rows (False for a batch none of whose members ends good);
    must_cluster: the cluster kernel must have taken tiles.
    -> the evidence, as a dict, for the record."""
    got = (st["n_mlp_fwd_launches"], st["n_mlp_jac_launches"], st["n_mlp_prepass_launches"])
    ev = dict(form=name, launches=got, n_render_rows=st["n_render_rows"], n_cluster_tiles=st["n_cluster_tiles"], prepass_mode=st["prepass_mode"],
              guard_trips=st["prepass_guard_trips"])
    print("evidence:", ev)
    assert st["prepass_guard_rerun"] == 0 and st["prepass_guard_trips"] == 0, (name, st["prepass_guard_trips"])
    assert st["prepass_mode"] == plan["prepass_mode"], (name, st["prepass_mode"])
    assert got == expected_launches(plan, fronts), (name, got, expected_launches(plan, fronts), plan)
    if plan["prepass_mode"] == 0:
        assert st["n_mlp_prepass_launches"] == 0 and st["n_prepass_points"] == 0, name
    else:
        assert st["n_mlp_prepass_launches"] > 0 and st["n_prepass_points"] > 0, name
    if rows_expected:
        assert (st["n_render_rows"] > 0) == bool(plan["mask_reuse"]), (name, st["n_render_rows"], plan["mask_reuse"])
    assert st["cluster_fallback"] == 0, name
    if must_cluster:          # the jacobian list is short enough for the cluster kernel to take it (at most cluster_max_tiles tiles)
        assert plan["cluster"] and st["n_cluster_tiles"] > 0, (name, st["n_cluster_tiles"])
    if not plan["cluster"]:
        assert st["n_cluster_tiles"] == 0, (name, st["n_cluster_tiles"])
    return ev
