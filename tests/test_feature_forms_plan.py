"""CPU-only: every named launch form of tests/launch_forms.py reaches the LaunchPlan fields it claims (csrc/launch_plan.h, evaluated by the
library's host hook at 256 CUs / 64 clusters) on every batch shape tests/test_gpu_feature_forms.py pins it on.  A form whose pins do not
produce its plan on a shape would make the device test compare the automatic plan with itself; this file is what catches that.  Every
row is printed (pytest -s): the table of profiles/feature_forms.md."""
import numpy as np
import pytest

import launch_forms as F
from test_launch_plan import PLAN


@pytest.fixture(scope="module")
def shapes():
    return F.shapes()


def _show(p):
    return {k: v for k, v in p.items() if v and k != "cluster_max_tiles"}


def test_the_shapes_are_what_the_device_tests_assume(shapes):
    s = shapes
    assert [s[k]["B"] for k in ("ragged3", "detection", "hinted3", "auto_block17", "metric3", "step6", "views18", "pose_pair")] == [3, 1, 3, 17, 3, 6, 18, 2]
    assert (s["detection"]["sum_pts"], s["detection"]["sum_rays"]) == (250, 450)
    assert (s["hinted3"]["sum_pts"], s["hinted3"]["sum_rays"], s["hinted3"]["D"]) == (450, 1050, 50)
    assert s["hinted3"]["cap_s"] / 128 > 1.5 * F.N_CU          # more than a round and a half of 128-point prepass tiles: hint passes, not one whole pass
    assert (s["auto_block17"]["sum_pts"], s["auto_block17"]["sum_rays"]) == (17 * 250, 17 * 60)
    assert s["ragged3_d64"]["D"] == 64 and s["ragged3"]["sum_pts"] == 120 + 97 + 150
    views = F.sizes(F.views18())
    assert len(views) == 18 and s["views18"]["grouped"]
    away = 3 * F.AWAY[0] + F.AWAY[1]
    assert views[away] == (50, 30)
    assert all(60 <= p <= 100 and 40 <= r <= 80 for i, (p, r) in enumerate(views) if i != away), views


def test_the_automatic_plans(shapes):
    """What nothing pinned gives on each shape -- the reference run of every device test."""
    auto = {k: F.plan_of(s) for k, s in shapes.items()}
    for k, p in auto.items():
        print("automatic %-14s %s" % (k, _show(p)))
    small = dict(bookkeeping_form=2, prepass_mode=1, guard_on=1, split_rows=1, reuse_throughput=0, kernel_timing=0)
    for k in ("ragged3", "ragged3_d64", "detection", "hinted3", "metric3", "step6"):
        assert all(auto[k][f] == v for f, v in small.items()), (k, auto[k])
    for k in ("ragged3", "detection"):          # the plan every feature test has run so far
        assert all(auto[k][f] == v for f, v in dict(speculative_band=1, cluster=1, whole=1, fixed_passes=1, lp_tile_pts=64).items()), (k, auto[k])
    assert auto["detection"]["direct_tiles"] == 1 and auto["ragged3"]["direct_tiles"] == 0
    for k in ("hinted3", "step6"):              # hint passes WITH the prepass, the mixed form of mask reuse
        assert all(auto[k][f] == v for f, v in dict(hint_passes=2, fixed_passes=0, whole=0, mixed_reuse=1, speculative_band=0, lp_tile_pts=128).items()), (k, auto[k])
    assert all(auto["auto_block17"][f] == v for f, v in dict(bookkeeping_form=0, reuse_throughput=1, mask_reuse=1, kernel_timing=1, hint_passes=2, jac_tile_pts=64,
                                                             prepass_mode=1, split_rows=0, tail_split=0).items()), auto["auto_block17"]
    assert all(auto["views18"][f] == v for f, v in dict(bookkeeping_form=0, kernel_timing=1, hint_passes=2, direct_tiles=0, prepass_mode=1).items()), auto["views18"]
    assert all(auto["pose_pair"][f] == v for f, v in dict(split_rows=1, cluster=1, prepass_mode=0, bookkeeping_form=0).items()), auto["pose_pair"]


def _cases(shapes):
    for name, s in shapes.items():
        for form in F.uses(name, s):
            yield name, s, form, None
    for form in F.F16_FORMS:
        yield "ragged3", shapes["ragged3"], form, F.F16_PINS


def test_every_form_reaches_its_plan_on_every_shape_it_is_pinned_on(shapes):
    bad = []
    for name, s, form, extra in _cases(shapes):
        p = F.plan_of_form(s, form, extra)
        want = dict(F.FORMS[form]["plan"])
        if extra:
            want.update(lp_compute=1, prepass_mode=1, jac_tile_pts=128)
        if s["pose_only"]:
            want.pop("fwd_tile_pts", None)
        if form == "prepass_off" and p["hint_passes"] == 3:
            want["hint_passes"] = 3
        miss = {k: (v, p[k]) for k, v in want.items() if p[k] != v}
        print("%-12s %-22s%s %s" % (name, form, " f16" if extra else "", _show(p)))
        if miss:
            bad.append((name, form, miss))
    assert not bad, bad


def test_every_form_changes_the_plan_somewhere(shapes):
    """Each form differs from the automatic plan on at least one shape it is pinned on (else it is the reference run under another name)."""
    changed = {}
    for name, s, form, extra in _cases(shapes):
        if extra is None:
            changed[form] = changed.get(form, False) or F.plan_of_form(s, form) != F.plan_of(s)
    assert set(changed) == set(F.FORMS), set(F.FORMS) - set(changed)
    # (direct tiles are what a one-object batch has by itself: the pin that changes the plan is direct_tiles_off)
    assert [k for k, v in changed.items() if not v] == ["direct_tiles_on"], [k for k, v in changed.items() if not v]


def test_the_multiview_table_of_pins_on_views18(shapes):
    """tests/test_gpu_multiview.FORMS as the device test applies it to the 18-view batch: each entry's plan.  Five of the nine leave the
    automatic plan of this batch as it is (18 members: block bookkeeping, tail tiles and the mixed form already, no speculative band, and the
    mixed form keeps the cluster form out) -- which is why the device test pins the named forms of tests/launch_forms.py on it as well."""
    import test_gpu_multiview as TM
    s, auto, same = shapes["views18"], F.plan_of(shapes["views18"]), []
    for pins in TM.FORMS:
        p = F.plan_of(s, {k[len("set_"):]: v for k, v in pins.items()})
        print("views18 %-45s %s" % (pins, _show(p)))
        if p == auto:
            same.append(pins)
    assert same == [dict(set_wave_bookkeeping=0), dict(set_tail_split=1, set_wave_bookkeeping=0), dict(set_cluster_tiles=1), dict(set_speculative_band=0),
                    dict(set_mixed_reuse=1)], same


def test_the_forms_reach_both_values_of_every_field(shapes):
    plans = np.array([[F.plan_of_form(s, form, extra)[k] for k in PLAN] for _, s, form, extra in _cases(shapes) if not s["pose_only"]])
    col = {k: plans[:, i] for i, k in enumerate(PLAN)}
    for k in ("bookkeeping_form", "speculative_band", "split_rows", "mixed_reuse", "reuse_throughput", "cluster", "tail_split", "direct_tiles", "whole", "split_fwd",
              "kernel_timing", "guard_on"):
        assert len(set(col[k].tolist())) == 2, (k, set(col[k].tolist()))
    assert set(col["prepass_mode"].tolist()) == {0, 1, 2} and set(col["lp_tile_pts"].tolist()) == {64, 128} and set(col["jac_tile_pts"].tolist()) == {16, 64, 128}
    assert (col["fixed_passes"] > 1).any() and (col["hint_passes"] > 0).any() and ((col["hint_passes"] > 0) & (col["prepass_mode"] == 0)).any()
    assert ((col["hint_passes"] > 0) & (col["prepass_mode"] > 0)).any() and ((col["fixed_passes"] == 10) & (col["prepass_mode"] > 0)).any()
    # the combinations the feature tests exist for: the bench's form, and block bookkeeping in front of the latency forms
    assert ((col["reuse_throughput"] == 1) & (col["bookkeeping_form"] == 0)).any() and ((col["bookkeeping_form"] == 0) & (col["split_rows"] == 1)).any()
    pose = [F.plan_of_form(shapes["pose_pair"], f) for f in F.uses("pose_pair", shapes["pose_pair"])]
    assert {(p["split_rows"], p["cluster"]) for p in pose} == {(1, 1), (1, 0), (0, 0)}


def test_expected_launches_follow_the_plan():
    plan = dict.fromkeys(PLAN, 0)
    assert F.expected_launches(dict(plan, prepass_mode=1, fixed_passes=1, whole=1, speculative_band=1), 4) == (0, 4, 4)
    assert F.expected_launches(dict(plan, prepass_mode=1, fixed_passes=10), 4) == (4, 4, 40)
    assert F.expected_launches(dict(plan, prepass_mode=1, hint_passes=2, reuse_throughput=1), 3) == (3, 6, 6)
    assert F.expected_launches(dict(plan, hint_passes=2), 3) == (6, 3, 0)
    assert F.expected_launches(dict(plan, split_rows=1), 8) == (0, 8, 0)          # pose-only
