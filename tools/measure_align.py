#!/usr/bin/env python3
"""What map alignment (dsp_map_align) costs next to what a caller could do before it existed, on one MI355X:

    python tools/measure_align.py [--reps 5] [--iterations 6] [--out profiles/map_align.md]

Shapes: the 300-point scene of tests/test_gpu_map_align.py (3 objects), 3 objects x 20 000 points, 64 objects x 100 000 points, each at 1,
4 and 16 hypotheses (starts 2 degrees / 0.02 off the true pose, tolerances 0, so every hypothesis makes every evaluation).  Reported per
shape: wall-clock ms per evaluation of the fused call (median of --reps calls after one warm-up, over the evaluations made), the decoder
launches' share of the call (HIP events on the handle's stream, dsp_debug_query_timing), decoder rows per tile, and the same loop as the
parent commit allows it: per hypothesis and iteration a numpy transform, Engine.query_map(normals=True), a numpy Gram with the unit normal
as the jacobian and a host solve.  `floor` is the fused call's ms per evaluation on an EIGHT-point cloud with the same map and hypotheses:
the launches, the two host synchronisations (candidate counts; sums) and the host step with next to no device work -- the upper bound of
what moving the 6 x 6 solve to the device could save per evaluation.  Also the recovery figures of the 300-point scene: pose error of the
device call and of tests/align_ref.py's loop run on the device's own decoder rows.  First measurements: recorded, nothing is gated on them.
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

F32, F64 = np.float32, np.float64
MAX_DIST, HUBER = 0.3, 0.05


def median_time(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def caller_loop(eng, t, codes, pts_s, T0, iterations):
    """One hypothesis as the parent commit allows it: upload and four downloads per iteration, the unit normal for the jacobian, no robust
    cost, no step rule."""
    T = np.array(T0, F64)
    for _ in range(iterations):
        pw = (pts_s.astype(F64) @ T[:3, :3].T + T[:3, 3]).astype(F32)
        r = eng.query_map(t, codes, pw, normals=True)
        use = (r["obj"] >= 0) & (np.abs(r["dist"]) <= MAX_DIST)
        if use.sum() < 6:
            break
        p, g, d = pw[use].astype(F64), r["normal"][use].astype(F64), r["dist"][use].astype(F64)
        J = np.concatenate([g, np.cross(p, g)], 1)
        xi = np.linalg.solve(J.T @ J + 1e-9 * np.eye(6), -(J.T @ d))
        th = math.sqrt(float(xi[3:] @ xi[3:]))
        K = np.array([[0, -xi[5], xi[4]], [xi[5], 0, -xi[3]], [-xi[4], xi[3], 0]])
        a, b, c = (1.0, 0.5, 1 / 6) if th < 1e-6 else (math.sin(th) / th, (1 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3)
        D = np.eye(4)
        D[:3, :3] = np.eye(3) + a * K + b * K @ K
        D[:3, 3] = (np.eye(3) + b * K + c * K @ K) @ xi[:3]
        T = D @ T
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) here")
    args = ap.parse_args()
    import align_ref as A
    import query_ref as Q
    import measure_query as MQ
    from dsp_slam_amd import fixtures, engine as E, _lib as L
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    lib = L.load()
    specs = fixtures.fixture_specs("cars")
    net = specs["NetworkSpecs"]
    layers = fold_weight_norm(fixtures.load_decoder_npz(fixtures.fixture_path("cars")), len(net["dims"]) + 1)
    eng = E.Engine(layers, net["latent_in"], specs.get("CodeLength", 64), device=0)
    T_true = A.rigid(A.axis_angle([0.3, -1.0, 0.5], 0.7), [0.5, -1.5, 2.0])
    inv = np.linalg.inv(T_true)
    to_sensor = lambda world: (np.asarray(world, F64) @ inv[:3, :3].T + inv[:3, 3]).astype(F32)

    # the 300-point scene, as in tests/test_gpu_map_align.py
    rng = np.random.default_rng(7)
    t3 = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [2.6, 0.3, -0.2], [4.0, -3.0, 1.0]])
    codes3 = list(rng.uniform(-0.3, 0.3, (3, 64)).astype(F32))
    start = []
    for _ in range(3):
        u = rng.normal(size=(600, 3))
        start.append((u / np.sqrt((u * u).sum(1))[:, None] * (0.5 * rng.uniform(0, 1, (600, 1)) ** (1 / 3))).astype(F32))
    start = [r["vertices"] for r in eng.surface_points(codes3, start, steps=8)]
    world = []
    for o, r in enumerate(eng.surface_points(codes3, start, steps=8)):
        p = r["vertices"].astype(F64)
        keep = p[(np.abs(r["sdf"]) < 1e-6) & (np.sqrt((p * p).sum(1)) < 0.9)][:100]
        world.append(keep @ t3[o, :3, :3].astype(F64).T + t3[o, :3, 3].astype(F64))
    world = np.concatenate(world)
    centre = world.mean(0)
    near, far = A.offset_pose(rng, T_true, 5.0, 0.05, centre), A.offset_pose(rng, T_true, 30.0, 0.3, centre)
    pts300 = to_sensor(world)
    kw = dict(max_dist=MAX_DIST, huber=HUBER, trans_tol=0.0, rot_tol=0.0)
    res = eng.align_to_map(t3, codes3, pts300, np.stack([near, far]), iterations=8, **kw)

    def decode(o, p):
        v, g = eng.sdf_jacobian(codes3[o], p)
        return v, g[:, -3:]
    ref = A.run(near, pts300, None, A.Map(t3, codes3), decode, iterations=8, **kw)
    dev_err, ref_err = A.pose_error(res["pose"][0], T_true), A.pose_error(ref["pose"], T_true)
    base_err = A.pose_error(caller_loop(eng, t3, codes3, pts300, near, 8), T_true)

    shapes = [("300-point scene", t3, codes3, pts300, centre)]
    for n_obj, n_pts in ((3, 20000), (64, 100000)):
        rng = np.random.default_rng(2000 + n_obj)
        t = MQ.make_map(rng, n_obj, False)
        codes = list(rng.uniform(-0.3, 0.3, (n_obj, 64)).astype(F32))
        w = MQ.make_points(rng, t, n_pts)
        shapes.append(("%d objects x %d points" % (n_obj, n_pts), t, codes, to_sensor(w), w.astype(F64).mean(0)))
    head = ["| shape | hypotheses | fused ms / evaluation | caller's loop ms / evaluation | ratio | decoder share | rows / tile | floor ms / evaluation | floor share |",
            "|---|---|---|---|---|---|---|---|---|"]
    lines, ratios = list(head), []
    for name, t, codes, pts, c in shapes:
        for n_hyp in (1, 4, 16):
            rng = np.random.default_rng(n_hyp)
            hyp = np.stack([A.offset_pose(rng, T_true, 2.0, 0.02, c) for _ in range(n_hyp)])
            run = lambda p=pts: eng.align_to_map(t, codes, p, hyp, iterations=args.iterations, **kw)
            r = run()
            evals = int(r["evaluations"].sum())
            t_new = median_time(run, args.reps)
            L.check(lib.dsp_debug_query_timing(eng._h, 1, None), eng._h, "dsp_debug_query_timing")
            run()
            ms = (C.c_double * 2)()
            L.check(lib.dsp_debug_query_timing(eng._h, 0, ms), eng._h, "dsp_debug_query_timing")
            st = eng.align_stats()
            # the floor cloud: eight points that hypothesis 0 used at its returned pose (fewer than min_points would end at the first evaluation)
            pp = eng.align_to_map(t, codes, pts, hyp[:1], iterations=args.iterations, per_point=True, **kw)
            few = pts[np.flatnonzero((pp["obj"][0] >= 0) & (np.abs(pp["dist"][0]) < 0.1))[:8]]
            t_floor = median_time(lambda: run(few), args.reps)
            n_ev_floor = max(1, eng.align_stats()["evaluations"])
            n_ev = max(1, st["evaluations"])
            t_old = median_time(lambda: [caller_loop(eng, t, codes, pts, hyp[k], args.iterations) for k in range(n_hyp)], max(1, args.reps // 2))
            per_new, per_old, per_floor = 1e3 * t_new / n_ev, 1e3 * t_old / n_ev, 1e3 * t_floor / n_ev_floor
            lines.append("| %s | %d | %.3f | %.3f | %.1fx | %.1f %% | %.1f | %.3f | %.1f %% |" % (
                name, n_hyp, per_new, per_old, per_old / per_new, 100 * ms[0] / ms[1] if ms[1] > 0 else float("nan"),
                st["rows"] / max(1, st["tiles"]), per_floor, 100 * per_floor / per_new))
            ratios.append(per_old / per_new)
            print(lines[-1], "(evaluations made by all hypotheses: %d, by the floor run: %d)" % (evals, n_ev_floor), flush=True)
    text = ["# Map alignment: dsp_map_align against the caller's own loop", "",
            "`python tools/measure_align.py --reps %d --iterations %d`, fixture decoder `cars`, one MI355X.  Wall-clock medians after one warm-up, "
            "host arrays in, host arrays out, %d evaluations per hypothesis (tolerances 0, starts 2 degrees / 0.02 off the true pose).  An "
            "evaluation here is one iteration of the call, all hypotheses together; the caller's loop runs the hypotheses one after the other "
            "and its time is divided by the same number.  The caller's loop is what the parent commit allows: per hypothesis and iteration a numpy "
            "transform, `Engine.query_map(normals=True)` (points up, four arrays down), a numpy Gram with the UNIT normal as the jacobian and a "
            "host solve -- no robust cost, no step rule.  `decoder share`: HIP events around the decoder launches over events around the whole "
            "call.  `floor`: the same call on an eight-point cloud (points the first hypothesis uses) -- launches, the two host synchronisations per evaluation and the host step with "
            "next to no device work; `floor share` = floor / fused.  It bounds what a device-side 6 x 6 solve could save per evaluation from above "
            "(the candidate counts' read-back would stay)." % (args.reps, args.iterations, args.iterations), ""] + lines + ["",
            "The fused call is %s the caller's loop at every measured shape: the ratio runs from %.1fx to %.1fx." % (
                "no slower than" if min(ratios) >= 1.0 else "NOT everywhere as fast as", min(ratios), max(ratios)), "",
            "## Recovery on the 300-point scene (8 evaluations from 5 degrees / 0.05)", "",
            "| | translation error | rotation error (rad) |", "|---|---|---|",
            "| dsp_map_align | %.3e | %.3e |" % dev_err,
            "| tests/align_ref.py's loop on the device's decoder rows | %.3e | %.3e |" % ref_err,
            "| the caller's loop (unit normal, no robust cost) | %.3e | %.3e |" % base_err, "",
            "With the 30 degrees / 0.3 hypothesis alongside: best = %d, its cost %.3e against %.3e (ratio %.3e), %d of 300 points used." % (
                res["best"], res["cost"][1], res["cost"][0], res["cost"][1] / res["cost"][0], res["n_used"][1]), ""]
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text))
    eng.close()


if __name__ == "__main__":
    main()
