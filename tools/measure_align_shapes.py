#!/usr/bin/env python3
"""What shape refinement (dsp_map_align_shapes) costs next to the object refinement it shares its cast with, and what it recovers, on one
MI355X:

    python tools/measure_align_shapes.py [--reps 9] [--objects 3 64 600] [--out profiles/map_align_shapes.md]

Time.  The maps of tools/measure_align_objects.py (3, 64 and 600 objects on a grid, about 100 rays per object, fixture decoder `cars`).
Wall-clock medians after a warm-up, each timed call ending in the call's own synchronisation, the two kinds of call ALTERNATED inside every
repeat: `objects` = align_objects_to_rays(iterations=1, per_ray=False), the yardstick on the same commit; `shapes` =
align_shapes_to_rays(iterations=1, per_ray=False, unknowns="pose+code").  One evaluation each.  With dsp_debug_query_timing on, a second
set of repeats splits every call's device time (events on the stream around the whole call) into the decoder launches of the cast and the
rest: the rest is where the 64 code derivatives per winner and the 70 x 70 Gram are.  Spread = (max - min) / median over the repeats.

Recovery.  The scene of tests/test_gpu_map_align_shapes.py::test_recovery (the `complex` fixture decoder, three objects at their true
poses, 50 rays per object from each of two sensor positions, start codes an unrelated uniform(-0.3, 0.3) draw): cost and depth RMS over the
matched rays per object at the start and after six evaluations, code only, damp 1e-4, with and without step control.  The float64 loop on
the oracle's decoder is printed by tests/test_align_shapes_host.py (-s).  First measurements: recorded, nothing is gated on them.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32, F64 = np.float32, np.float64
MAX_DIST, HUBER, MAX_GAP = 0.3, 0.05, 0.6
PER_OBJ = 100
STEP = (1e-3, 10.0, 0.1, 1e-9, 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--objects", type=int, nargs="+", default=[3, 64, 600])
    ap.add_argument("--out", default=None, help="also write the tables (markdown) here")
    args = ap.parse_args()
    import align_ref as A
    import query_ref as Q
    import test_align_objects_host as H
    from test_align_rays_host import aimed_rays
    from dsp_slam_amd import fixtures, engine as E, _lib as L
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm

    def engine(name):
        specs = fixtures.fixture_specs(name)
        net = specs["NetworkSpecs"]
        layers = fold_weight_norm(fixtures.load_decoder_npz(fixtures.fixture_path(name)), len(net["dims"]) + 1)
        return E.Engine(layers, net["latent_in"], specs.get("CodeLength", 64), device=0)

    kw = dict(max_dist=MAX_DIST, huber=HUBER, trans_tol=0.0, rot_tol=0.0, max_gap=MAX_GAP, raycast=dict(max_steps=64))

    def observe(eng, t, codes, sensors, per_obj, aim):
        """world end points and origins: every sensor aims `aim` rays at each of its objects; the first per_obj hits of each are kept"""
        pw, ow = [], []
        for T, objs in sensors:
            dirs = aimed_rays(np.random.default_rng(len(pw) + 1), t[objs], T, aim)
            dirs_w = (dirs @ T[:3, :3].T).astype(F32)
            org = np.broadcast_to(T[:3, 3].astype(F32), dirs_w.shape).copy()
            c = eng.cast_rays(t, codes, org, dirs_w, eps=1e-5, max_steps=256)
            for o in objs:
                k = np.flatnonzero((c["obj"] == o) & (c["status"] == 1))[:per_obj]
                u = dirs_w[k].astype(F64)
                u /= np.sqrt((u * u).sum(1))[:, None]
                pw.append((org[k].astype(F64) + u * c["t"][k].astype(F64)[:, None]).astype(F32))
                ow.append(org[k])
        return np.concatenate(pw), np.concatenate(ow)

    def depth_rms(res, pw, ow, n_obj):
        length = np.sqrt(((pw.astype(F64) - ow.astype(F64)) ** 2).sum(1))
        return [float(np.sqrt(((length[res["obj"] == k] - res["t"][res["obj"] == k].astype(F64)) ** 2).mean())) if (res["obj"] == k).any() else float("nan")
                for k in range(n_obj)]

    # ---- recovery (the `complex` decoder) ----
    eng = engine("complex")
    rng = np.random.default_rng(H.SEED)
    t_true, codes = H.layout(rng)
    codes = list(codes)
    pw, ow = observe(eng, t_true, codes, [(T, [0, 1, 2]) for T in H.SENSORS], H.PER_OBJ, 4 * H.PER_OBJ)
    start = list(np.random.default_rng(77).uniform(-0.3, 0.3, (3, 64)).astype(F32))
    first = eng.align_shapes_to_rays(t_true, start, pw, ow, iterations=1, per_ray=True, **kw)
    rms0 = depth_rms(first, pw, ow, 3)
    rec = ["| object | run | cost: start -> returned (ratio) | depth RMS over matched rays: start -> returned | rays used | steps | status |", "|---|---|---|---|---|---|---|"]
    for name, extra in (("plain Gauss-Newton", {}), ("step control %s" % (STEP,), dict(step_control=STEP))):
        res = eng.align_shapes_to_rays(t_true, start, pw, ow, iterations=6, per_ray=True, unknowns="code", damp=1e-4, code_tol=0.0, **kw, **extra)
        rms1 = depth_rms(res, pw, ow, 3)
        for k in range(3):
            rec.append("| %d | %s | %.2e -> %.2e (%.3f) | %.4f -> %.4f | %d | %d | %d |" % (
                k, name, res["cost0"][k], res["cost"][k], res["cost"][k] / res["cost0"][k], rms0[k], rms1[k], res["n_used"][k], res["steps"][k], res["status"][k]))
            print(rec[-1], flush=True)
    eng.close()

    # ---- time (the `cars` decoder) ----
    eng = engine("cars")
    lib = L.load()
    codes3 = list(np.random.default_rng(7).uniform(-0.3, 0.3, (3, 64)).astype(F32))
    tim = ["| objects | rays | objects ms | shapes ms | ratio | device ms objects: decoder / rest | device ms shapes: decoder / rest | pairs | march rows | "
           "spread objects / shapes |", "|---|---|---|---|---|---|---|---|---|---|"]
    for n_obj in args.objects:
        r = np.random.default_rng(n_obj)
        side = int(np.ceil(np.sqrt(n_obj)))
        centres = np.array([[3.2 * (k % side), 3.2 * (k // side), 0.0] for k in range(n_obj)])
        t = Q.sim3(Q.random_rotations(r, n_obj), r.uniform(0.6, 1.3, n_obj), centres)
        cs = [codes3[k % 3] for k in range(n_obj)]
        sensors = []
        for k in range(n_obj):
            z = np.array([0.0, 0.35, -0.94])
            z /= np.sqrt((z * z).sum())
            x = np.cross([0.0, 1.0, 0.0], z)
            x /= np.sqrt((x * x).sum())
            sensors.append((A.rigid(np.stack([x, np.cross(z, x), z], 1), centres[k] - 4.0 * z), [k]))
        pw, ow = observe(eng, t, cs, sensors, PER_OBJ, int(2.5 * PER_OBJ))
        t_start = np.stack([A.offset_pose(r, x.astype(F64), 3.0, 0.03, x[:3, 3].astype(F64)) for x in t]).astype(F32)
        f_objects = lambda: eng.align_objects_to_rays(t_start, cs, pw, ow, iterations=1, **kw)
        f_shapes = lambda: eng.align_shapes_to_rays(t_start, cs, pw, ow, iterations=1, unknowns="pose+code", **kw)
        fs = (f_objects, f_shapes)
        for f in fs:
            f()
        ts = {f: [] for f in fs}
        for _ in range(args.reps):
            for f in fs:
                c0 = time.perf_counter()
                f()
                ts[f].append(time.perf_counter() - c0)
        med = {f: 1e3 * float(np.median(v)) for f, v in ts.items()}
        spread = {f: (max(v) - min(v)) / float(np.median(v)) for f, v in ts.items()}
        st = eng.align_shapes_stats()
        dev = {f: [] for f in fs}
        ms2 = np.zeros(2, F64)
        assert lib.dsp_debug_query_timing(eng._h, 1, None) == 0
        try:
            for _ in range(args.reps):
                for f in fs:
                    f()
                    assert lib.dsp_debug_query_timing(eng._h, 1, L.ptr(ms2, L.c_f64p)) == 0
                    dev[f].append(ms2.copy())
        finally:
            assert lib.dsp_debug_query_timing(eng._h, 0, None) == 0
        split = {f: np.median(np.stack(v), 0) for f, v in dev.items()}
        tim.append("| %d | %d | %.3f | %.3f | %.2f | %.3f / %.3f | %.3f / %.3f | %d | %d | %.0f %% / %.0f %% |" % (
            n_obj, pw.shape[0], med[f_objects], med[f_shapes], med[f_shapes] / med[f_objects], split[f_objects][0], split[f_objects][1] - split[f_objects][0],
            split[f_shapes][0], split[f_shapes][1] - split[f_shapes][0], st["pairs"], st["rows"], 100 * spread[f_objects], 100 * spread[f_shapes]))
        print(tim[-1], flush=True)
    eng.close()
    text = ["# Shape refinement: dsp_map_align_shapes", "",
            "What the call is: `include/dsp_gn.h`, DESIGN.md \"Shape refinement\"; the arithmetic: `dsp_slam_amd/csrc/align_shapes_math.h`.  Written by",
            "`tools/measure_align_shapes.py` on one MI355X.  Nothing is gated on any figure here.  The float64 loop on the oracle's decoder (the same",
            "scene, the algorithm without the device) is printed by `tests/test_align_shapes_host.py -s`.", "",
            "## 1. Recovery on the device (the scene of `tests/test_gpu_map_align_shapes.py::test_recovery`)", "",
            "Decoder `complex`, three objects at their true poses, 50 rays per object from each of two sensor positions, start codes an unrelated",
            "uniform(-0.3, 0.3) draw; six evaluations, code only, `damp` 1e-4 on the mean system, no regulariser, `max_gap` %.1f.  The distance between" % MAX_GAP,
            "the returned and the true code is not reported: two views leave most code directions unobserved.", ""] + rec + [
        "", "## 2. Time of one evaluation (`--reps %d`, decoder `cars`, about %d rays per object)" % (args.reps, PER_OBJ), "",
        "`objects`: `dsp_map_align_objects`, `shapes`: `dsp_map_align_shapes` with pose and code unknowns, on the same rays and map, alternated.",
        "Wall-clock ms per call (median), then the device time of a call from stream events, split into the cast's decoder launches and the rest",
        "(bookkeeping kernels, the 256 B of code derivatives per winner, the Gram, the waits for the host between them).", ""] + tim + [""]
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text))


if __name__ == "__main__":
    main()
