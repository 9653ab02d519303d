"""CPU-only: the launch plan (dsp_slam_amd/csrc/launch_plan.h: which of the bit-identical forms of each computation a run uses) against a
table of (inputs, plan) rows recorded from the sixteen predicates that function replaced.

tests/golden/launch_plan_table.npz was recorded at the commit before the plan existed: profiles/launch_plan_record.patch adds a
throw-away hook to that commit's library which fills a host-side batch / handle from each input row and calls the old predicates,
unmodified, and a script that feeds it `build_rows()` below.  Never regenerate it from make_launch_plan.

The library evaluates the plan through dsp_debug_launch_plan (a host-only test hook, not declared in include/dsp_gn.h)."""
import os

import numpy as np
import pytest

from dsp_slam_amd import _lib as L

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan_table.npz")

# the order of the hook's integer arrays (dsp_gn.hip: dsp_debug_launch_plan)
INPUTS = ("pose_only", "B", "D", "sum_pts", "sum_rays", "cap_s", "split_rows", "mask_reuse", "mixed_reuse", "speculative", "fused_bookkeeping",
          "tail_split", "cluster_tiles", "direct_tiles", "compute", "lp_small", "prepass", "lp_tile", "prepass_guard", "kernel_timing",
          "n_ray_passes", "n_pass_bounds", "n_bound_ranges", "n_cu", "n_clusters", "lp_ok", "lpj_ok", "cl_cooldown")
PLAN = ("kernel_timing", "lp_compute", "reuse_throughput", "bookkeeping_form", "prepass_mode", "guard_on", "speculative_band", "split_rows",
        "mixed_reuse", "mask_reuse", "cluster", "cluster_max_tiles", "split_fwd", "tail_split", "lp_tile_pts", "fwd_tile_pts", "jac_tile_pts",
        "direct_tiles", "fixed_passes", "hint_passes", "whole", "explicit_bounds")
I = {n: i for i, n in enumerate(INPUTS)}
P = {n: i for i, n in enumerate(PLAN)}

# settings a caller pins (-1 = automatic) and the values a pin can take
TRI = {"split_rows": (0, 1), "mask_reuse": (0, 1), "mixed_reuse": (0, 1), "speculative": (0, 1), "fused_bookkeeping": (0, 2), "tail_split": (0, 1),
       "cluster_tiles": (0, 1), "direct_tiles": (0, 1), "lp_small": (0, 1), "kernel_timing": (0, 1)}
CHIPS = ((256, 64), (24, 0))       # (n_cu, n_clusters = n_cu / 32 * 8): an MI355X, and a chip too small for the cluster form


def shape(B, pts, rays, D, pose_only=False):
    """B equal objects; sample slots are rounded up to 64 per object (batch_build)."""
    if pose_only:
        return dict(pose_only=1, B=B, D=2, sum_pts=B * pts, sum_rays=0, cap_s=0)
    return dict(pose_only=0, B=B, D=D, sum_pts=B * pts, sum_rays=B * rays, cap_s=B * (-(-rays * D // 64) * 64))


# shapes the comments of launch_plan.h say land on different forms; cfg2 / cfg5 with 500 rays per object, and (bench_*) as
# bench.py builds them (one ray per surface point + 500 background rays)
NAMED = [("kitti_detection", shape(1, 250, 450, 50)), ("cfg2_object", shape(1, 2000, 500, 50))]
NAMED += [("cfg2_x%d" % B, shape(B, 2000, 500, 50)) for B in (4, 8, 16, 17, 32, 64)]
NAMED += [("cfg5_batch", shape(32, 4000, 500, 50)), ("pose_only", shape(1, 250, 0, 2, pose_only=True)), ("pose_only_x64", shape(64, 2000, 0, 2, pose_only=True)),
          ("bench_cfg2_object", shape(1, 2000, 2500, 50)), ("bench_cfg2_x64", shape(64, 2000, 2500, 50)), ("bench_cfg5_half", shape(32, 4000, 4500, 50))]


def base_row(sh, n_cu=256, n_clusters=64):
    r = dict.fromkeys(INPUTS, -1)
    r.update(compute=0, prepass_guard=1, n_ray_passes=0, n_pass_bounds=0, n_bound_ranges=0, n_cu=n_cu, n_clusters=n_clusters, lp_ok=1, lpj_ok=1, cl_cooldown=0)
    r.update(sh)
    return r


def build_rows():
    """(names, int32 [n, len(INPUTS)]): the named shapes under every combination the plan's branches look at, then seeded random rows."""
    rows, names = [], []

    def add(name, r, **kw):
        r = dict(r, **kw)
        rows.append([r[k] for k in INPUTS])
        names.append(name)

    for name, sh in NAMED:
        for n_cu, n_cl in CHIPS:
            b = base_row(sh, n_cu, n_cl)
            for compute in (0, 1, 2):
                for prepass in (-1, 0, 1, 2):
                    for lp_ok, lpj_ok in ((1, 1), (1, 0), (0, 0)):        # (the 16-bit jacobian kernels need the prepass kernel's geometry: never 0, 1)
                        for cool in (0, 5):
                            add(name, b, compute=compute, prepass=prepass, lp_ok=lp_ok, lpj_ok=lpj_ok, cl_cooldown=cool)
            for key, pins in TRI.items():
                for v in pins:
                    for compute in (0, 1):
                        for prepass in (-1, 0):
                            add(name, b, compute=compute, prepass=prepass, **{key: v})
            for prepass in (-1, 0):
                for lp_tile in (64, 128):
                    add(name, b, prepass=prepass, lp_tile=lp_tile)
                add(name, b, prepass=prepass, prepass_guard=0)
                for n in (1, 2, 10, 64):
                    add(name, b, prepass=prepass, n_ray_passes=n)
                for n, k in ((2, 1), (2, 2), (3, 1), (10, 4)):          # explicit bounds: n ranges, k of them not empty
                    add(name, b, prepass=prepass, n_ray_passes=n, n_pass_bounds=n + 1, n_bound_ranges=k)
                add(name, b, prepass=prepass, n_ray_passes=64, n_pass_bounds=65, n_bound_ranges=3)      # more passes than depths: the bounds are dropped
    rng = np.random.default_rng(20261016)
    for _ in range(2000):
        pose = rng.random() < 0.1
        B = int(rng.choice([1, 1, 2, 3, 4, 8, 15, 16, 17, 24, 32, 64, int(rng.integers(1, 200))]))
        pts = int(rng.integers(20, 5000))
        sh = shape(B, pts, 0, 2, True) if pose else shape(B, pts, int(rng.integers(20, 5000)), int(rng.choice([2, 8, 30, 50, 64])))
        n_cu = int(rng.choice([256, 256, 304, 128, 64, 24]))
        r = base_row(sh, n_cu, n_cu // 32 * 8)
        for key, pins in TRI.items():
            if rng.random() < 0.25:
                r[key] = int(rng.choice(pins))
        r["compute"] = 0 if pose else int(rng.choice([0, 0, 1, 2]))
        r["prepass"] = int(rng.choice([-1, -1, 0, 1, 2]))
        r["lp_tile"] = int(rng.choice([-1, -1, 64, 128]))
        r["prepass_guard"] = int(rng.random() < 0.8)
        r["lp_ok"], r["lpj_ok"] = [(1, 1), (1, 1), (1, 0), (0, 0)][int(rng.integers(4))]
        r["cl_cooldown"] = int(rng.choice([0, 0, 1, 64]))
        if rng.random() < 0.3:
            r["n_ray_passes"] = int(rng.integers(1, 65))
            if rng.random() < 0.3:
                r["n_pass_bounds"] = r["n_ray_passes"] + 1
                r["n_bound_ranges"] = int(rng.integers(1, min(r["n_ray_passes"], r["D"]) + 1))
        add("random", r)
    return np.array(names), np.array(rows, dtype=np.int32)


@pytest.fixture(scope="module")
def table():
    t = np.load(TABLE)
    return t["names"], t["inputs"], t["plan"]


def evaluate(inputs):
    lib = L.load()
    fn = lib.dsp_debug_launch_plan
    out = np.zeros((len(inputs), len(PLAN)), dtype=np.int32)
    for i, row in enumerate(np.ascontiguousarray(inputs, dtype=np.int32)):
        assert fn(row.ctypes.data_as(L.c_i32p), len(INPUTS), out[i].ctypes.data_as(L.c_i32p), len(PLAN)) == 0, "row %d rejected" % i
    return out


def test_table_is_the_generators(table):
    names, inputs, plan = table
    gn, gi = build_rows()
    assert inputs.dtype == np.int32 and plan.dtype == np.int32 and plan.shape == (len(inputs), len(PLAN))
    assert np.array_equal(names, gn) and np.array_equal(inputs, gi)
    assert 2000 <= len(inputs) <= 20000 and os.path.getsize(TABLE) < 256 * 1024


def test_plan_replays_the_recorded_table(table):
    names, inputs, plan = table
    got = evaluate(inputs)
    bad = np.nonzero((got != plan).any(axis=1))[0]
    msg = ""
    if len(bad):
        i = bad[0]
        msg = "%d rows differ; first: row %d (%s) %s: %s" % (len(bad), i, names[i], dict(zip(INPUTS, inputs[i].tolist())), {
            k: (int(plan[i, j]), int(got[i, j])) for j, k in enumerate(PLAN) if plan[i, j] != got[i, j]})
    assert not len(bad), msg


def test_hook_rejects_malformed_rows(table):
    lib = L.load()
    fn = lib.dsp_debug_launch_plan
    row = np.array(table[1][0], dtype=np.int32)
    out = np.zeros(len(PLAN), dtype=np.int32)
    assert fn(row.ctypes.data_as(L.c_i32p), len(INPUTS) - 1, out.ctypes.data_as(L.c_i32p), len(PLAN)) != 0
    assert fn(row.ctypes.data_as(L.c_i32p), len(INPUTS), out.ctypes.data_as(L.c_i32p), len(PLAN) + 1) != 0
    row[I["lp_ok"]], row[I["lpj_ok"]] = 0, 1
    assert fn(row.ctypes.data_as(L.c_i32p), len(INPUTS), out.ctypes.data_as(L.c_i32p), len(PLAN)) != 0


def automatic(inputs):
    """rows in which nothing is pinned: every tri-state, the prepass, its tile and the passes automatic, the guard on (the compute mode is the
    caller's opt-in, the chip and the decoder's capabilities belong to the handle: any)"""
    m = np.ones(len(inputs), dtype=bool)
    for k in list(TRI) + ["prepass", "lp_tile"]:
        m &= inputs[:, I[k]] == -1
    return m & (inputs[:, I["n_ray_passes"]] == 0) & (inputs[:, I["n_pass_bounds"]] == 0) & (inputs[:, I["prepass_guard"]] == 1)


def test_table_reaches_every_value_with_automatic_settings(table):
    _, inputs, plan = table
    a = plan[automatic(inputs)]
    assert len(a) >= 100
    want = {k: (0, 1) for k in ("kernel_timing", "reuse_throughput", "guard_on", "speculative_band", "split_rows", "mixed_reuse", "mask_reuse", "cluster",
                                "split_fwd", "tail_split", "direct_tiles", "whole")}
    want.update(lp_compute=(0, 1, 2), bookkeeping_form=(0, 2), prepass_mode=(0, 1, 2), lp_tile_pts=(64, 128), fwd_tile_pts=(16, 64), jac_tile_pts=(16, 64, 128),
                fixed_passes=(0, 1, 10), hint_passes=(0, 2, 3), cluster_max_tiles=(0, 128))
    missing = {k: [v for v in vs if not (a[:, P[k]] == v).any()] for k, vs in want.items()}
    assert not any(missing.values()), {k: v for k, v in missing.items() if v}
    assert set(np.unique(plan[:, P["explicit_bounds"]]).tolist()) == {0, 1}      # (explicit bounds are a pin by definition)


def test_cross_form_conditions_hold_in_every_row(table):
    _, inputs, plan = table
    p = {k: plan[:, j] for k, j in P.items()}
    on = {k: v != 0 for k, v in p.items()}

    def implies(a, b, what):
        bad = np.nonzero(a & ~b)[0]
        assert not len(bad), "%s: row %d %s" % (what, bad[0], dict(zip(PLAN, plan[bad[0]].tolist())))

    implies(on["speculative_band"], (p["bookkeeping_form"] == 2) & on["prepass_mode"] & ~on["reuse_throughput"] & ~on["lp_compute"],
            "speculative band rows imply wave bookkeeping and the prepass, on the fp32 latency path")
    implies(on["cluster"], on["split_rows"] & ~on["mixed_reuse"], "the cluster form implies the latency form and excludes the mixed form")
    implies(on["mixed_reuse"], on["split_rows"] & ~on["speculative_band"], "the mixed form lives in the latency-form jacobian launch")
    implies(on["reuse_throughput"], ~(on["split_rows"] | on["split_fwd"] | on["tail_split"] | on["cluster"] | on["mixed_reuse"] | on["speculative_band"]),
            "throughput mask reuse excludes every latency form")
    assert np.array_equal(on["mask_reuse"], on["reuse_throughput"] | on["mixed_reuse"])
    implies(on["lp_compute"], (p["prepass_mode"] == p["lp_compute"]) & ~on["guard_on"] & ~on["mask_reuse"] & ~on["split_rows"] & ~on["cluster"] & ~on["split_fwd"] &
            ~on["tail_split"] & ~on["speculative_band"] & ~on["direct_tiles"] & (p["lp_tile_pts"] == 128) & (p["jac_tile_pts"] == 128),
            "the compute mode switches every fp32 form and the guard off")
    implies(on["split_fwd"], ~on["tail_split"], "no tail tiles behind a forward launch that is in the latency form already")
    implies(on["direct_tiles"], p["bookkeeping_form"] == 2, "direct tile lists need the wave form")
    implies(on["whole"], on["prepass_mode"] & (p["fixed_passes"] >= 1), "one pass over every sample in place is a prepass launch")
    implies(on["guard_on"], on["prepass_mode"], "the guard guards the prepass")
    render = inputs[:, I["pose_only"]] == 0
    implies(render, on["fixed_passes"] != on["hint_passes"], "fixed or hint-steered passes, never both")
    implies(~render, ~(on["lp_compute"] | on["prepass_mode"] | on["mask_reuse"] | on["bookkeeping_form"] | on["speculative_band"] | on["split_fwd"] |
                       on["tail_split"] | on["fixed_passes"] | on["hint_passes"] | on["direct_tiles"]), "a pose-only batch has no rays")
    assert np.array_equal(p["fwd_tile_pts"], np.where(on["split_fwd"], 16, 64))
    assert np.array_equal(p["jac_tile_pts"], np.where(on["lp_compute"], 128, np.where(on["split_rows"], 16, 64)))
    assert np.array_equal(p["cluster_max_tiles"], 2 * inputs[:, I["n_clusters"]])
