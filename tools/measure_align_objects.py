#!/usr/bin/env python3
"""What object refinement (dsp_map_align_objects) costs next to the sensor-side ray alignment it shares its cast with, and how close it
gets, on one MI355X:

    python tools/measure_align_objects.py [--reps 9] [--objects 3 64 600] [--out FILE.md]

Time.  Maps of 3, 64 and 600 objects on a grid (spacing 3.2, scales 0.6 .. 1.3, the three codes of the tests in turn), every object seen
by about 100 rays from a sensor position of its own 4 units away (observations: Engine.cast_rays of the whole map at eps 1e-5; the rays of
all sensors are concatenated).  Wall-clock medians after a warm-up, each timed call ending in the call's own synchronisation, the two kinds
of call ALTERNATED inside every repeat: `sensor` = align_rays_to_map(iterations=1) with ONE hypothesis (the identity: the world rays are
the sensor's) on the same rays and map -- the same cast with the unsegmented Gram, the parent commit's code path and the yardstick;
`objects` = align_objects_to_rays(iterations=1, per_ray=False).  Spread = (max - min) / median over the repeats.  Work counts from
Engine.align_objects_stats().

Recovery.  The scene of tests/test_gpu_map_align_objects.py::test_recovery (three objects displaced by 5, 12 and 20 degrees about their
centres, rays from two sensor positions): final pose errors per object on the device and in the restatement's loop
(tests/align_objects_ref.py through the engine's decoder), 8 evaluations.  The float64 loop on the oracle's decoder is printed by
tests/test_align_objects_host.py.  First measurements: recorded, nothing is gated on them.
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--objects", type=int, nargs="+", default=[3, 64, 600])
    ap.add_argument("--out", default=None, help="also write the tables (markdown) here")
    args = ap.parse_args()
    import align_objects_ref as AO
    import align_ref as A
    import query_ref as Q
    import test_align_objects_host as H
    from test_align_rays_host import aimed_rays
    from dsp_slam_amd import fixtures, engine as E
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    specs = fixtures.fixture_specs("cars")
    net = specs["NetworkSpecs"]
    layers = fold_weight_norm(fixtures.load_decoder_npz(fixtures.fixture_path("cars")), len(net["dims"]) + 1)
    eng = E.Engine(layers, net["latent_in"], specs.get("CodeLength", 64), device=0)
    kw = dict(max_dist=MAX_DIST, huber=HUBER, trans_tol=0.0, rot_tol=0.0, max_gap=MAX_GAP, raycast=dict(max_steps=64))
    codes3 = list(np.random.default_rng(7).uniform(-0.3, 0.3, (3, 64)).astype(F32))

    def observe(t, codes, sensors, per_obj):
        """world end points and origins: every sensor aims 2.5 x per_obj rays at its objects; the first per_obj hits of each are kept"""
        pw, ow = [], []
        for T, objs in sensors:
            dirs = aimed_rays(np.random.default_rng(len(pw) + 1), t[objs], T, int(2.5 * per_obj))
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

    # ---- recovery ----
    rng = np.random.default_rng(H.SEED)
    t_true, codes = H.layout(rng)
    codes = list(codes)
    pw, ow = observe(t_true, codes, [(T, [0, 1, 2]) for T in H.SENSORS], H.PER_OBJ)
    t0 = H.displaced(rng, t_true)
    rec = ["| object | start: translation / rotation (rad) | device | restatement's loop | rays used | status |", "|---|---|---|---|---|---|"]
    res = eng.align_objects_to_rays(t0, codes, pw, ow, iterations=8, **kw)
    ref = AO.run(3, AO.evaluator(eng, t0, codes, pw, ow, None, HUBER, MAX_DIST, MAX_GAP, dict(max_steps=64)), iterations=8, max_dist=MAX_DIST, huber=HUBER,
                 trans_tol=0.0, rot_tol=0.0)
    for k in range(3):
        tt = t_true[k].astype(F64)
        s, d, r = A.pose_error(t0[k].astype(F64), tt), A.pose_error(res["t_world_obj"][k].astype(F64), tt), A.pose_error(
            AO.compose(ref[k]["correction"], t0[k]).astype(F64), tt)
        rec.append("| %d (%g degrees / %g) | %.2e / %.2e | %.2e / %.2e | %.2e / %.2e | %d | %d |" % (
            k, H.OFFSETS[k][0], H.OFFSETS[k][1], s[0], s[1], d[0], d[1], r[0], r[1], res["n_used"][k], res["status"][k]))
        print(rec[-1], flush=True)

    # ---- time ----
    tim = ["| objects | rays | sensor (1 hypothesis) ms | objects ms | ratio | pairs | march rows | tiles | rounds | spread sensor / objects |",
           "|---|---|---|---|---|---|---|---|---|---|"]
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
        pw, ow = observe(t, cs, sensors, PER_OBJ)
        t_start = np.stack([A.offset_pose(r, x.astype(F64), 3.0, 0.03, x[:3, 3].astype(F64)) for x in t]).astype(F32)
        f_sensor = lambda: eng.align_rays_to_map(t_start, cs, pw, np.eye(4)[None], origins=ow, iterations=1, **kw)
        f_objects = lambda: eng.align_objects_to_rays(t_start, cs, pw, ow, iterations=1, **kw)
        for f in (f_sensor, f_objects):
            f()
        ts = {f: [] for f in (f_sensor, f_objects)}
        for _ in range(args.reps):
            for f in (f_sensor, f_objects):
                c0 = time.perf_counter()
                f()
                ts[f].append(time.perf_counter() - c0)
        med = {f: 1e3 * float(np.median(v)) for f, v in ts.items()}
        spread = {f: (max(v) - min(v)) / float(np.median(v)) for f, v in ts.items()}
        st = eng.align_objects_stats()
        tim.append("| %d | %d | %.3f | %.3f | %.2f | %d | %d | %d | %d | %.0f %% / %.0f %% |" % (
            n_obj, pw.shape[0], med[f_sensor], med[f_objects], med[f_objects] / med[f_sensor], st["pairs"], st["rows"], st["tiles"], st["rounds"],
            100 * spread[f_sensor], 100 * spread[f_objects]))
        print(tim[-1], flush=True)
    text = ["## Recovery on the device (the scene of `tests/test_gpu_map_align_objects.py::test_recovery`, 8 evaluations, max_gap %.1f)" % MAX_GAP, ""] + rec + [
        "", "## Time of one evaluation (`python tools/measure_align_objects.py --reps %d`, fixture decoder `cars`, one MI355X)" % args.reps, ""] + tim + [""]
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text))
    eng.close()


if __name__ == "__main__":
    main()
