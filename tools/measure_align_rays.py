#!/usr/bin/env python3
"""What ray alignment (dsp_map_align_rays) costs next to the cast it is built around, and how close it gets, on one MI355X:

    python tools/measure_align_rays.py [--reps 9] [--out FILE.md]

Time.  Two shapes on the three-object scene of tests/test_gpu_map_align_rays.py: 450 rays x 8 hypotheses (a KITTI-size object cloud and a
relocaliser's seeds) and a 160 x 120 depth image x 1 hypothesis (every pixel a ray, the background at a constant depth behind the
objects).  Per shape, wall-clock medians after a warm-up, each timed call ending in the call's own synchronisation, the three kinds of
call ALTERNATED inside every repeat: `cast` = Engine.cast_rays(normals=True) of the same H x N world rays (host rays up, five arrays down:
the yardstick, the parent commit's code path); `evaluation` = align_rays_to_map(iterations=1); `call` = align_rays_to_map with 8
evaluations (tolerances 0).  Spread = (max - min) / median over the repeats.

Accuracy.  The 300-ray scene from the 5 and the 20 degree start (8 and 12 evaluations) at eps 1e-3 and 1e-4, next to Engine.align_to_map
on the same points from the same starts.  First measurements: recorded, nothing is gated on them.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) here")
    args = ap.parse_args()
    import align_rays_ref as AR
    import align_ref as A
    import query_ref as Q
    from test_align_rays_host import aimed_rays
    from dsp_slam_amd import fixtures, engine as E, map_objects as M
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    specs = fixtures.fixture_specs("cars")
    net = specs["NetworkSpecs"]
    layers = fold_weight_norm(fixtures.load_decoder_npz(fixtures.fixture_path("cars")), len(net["dims"]) + 1)
    eng = E.Engine(layers, net["latent_in"], specs.get("CodeLength", 64), device=0)
    T_true = A.rigid(A.axis_angle([0.3, -1.0, 0.5], 0.7), [0.5, -1.5, 2.0])
    rng = np.random.default_rng(7)
    t = Q.sim3(Q.random_rotations(rng, 3), [0.8, 1.3, 0.6], [[0.0, 0.0, 0.0], [2.6, 0.3, -0.2], [4.0, -3.0, 1.0]])
    codes = list(rng.uniform(-0.3, 0.3, (3, 64)).astype(F32))

    def observe(T, dirs_s, background=None):
        """sensor-frame end points of the rays along dirs_s: the cast at the pose T (eps 1e-5); misses dropped, or put at depth `background`"""
        dirs_w = (dirs_s @ T[:3, :3].T).astype(F32)
        org_w = np.broadcast_to(T[:3, 3].astype(F32), dirs_w.shape).copy()
        c = eng.cast_rays(t, codes, org_w, dirs_w, eps=1e-5, max_steps=256)
        u = dirs_s / np.sqrt((dirs_s * dirs_s).sum(1))[:, None]
        hit = c["obj"] >= 0
        if background is None:
            return (u[hit] * c["t"][hit].astype(F64)[:, None]).astype(F32)
        return (u * np.where(hit, c["t"].astype(F64), background)[:, None]).astype(F32)

    pts_all = observe(T_true, aimed_rays(rng, t, T_true, 250))
    world = pts_all.astype(F64) @ T_true[:3, :3].T + T_true[:3, 3]
    centre = world.mean(0)
    kw = dict(max_dist=MAX_DIST, huber=HUBER, trans_tol=0.0, rot_tol=0.0)

    # ---- accuracy ----
    pts300 = pts_all[np.random.default_rng(1).permutation(pts_all.shape[0])[:300]]
    acc = ["| start | evaluations | eps | rays: translation / rotation (rad) | used | point aligner: translation / rotation (rad) | used |", "|---|---|---|---|---|---|---|"]
    r7 = np.random.default_rng(70)
    for name, deg, tr, iters in (("5 degrees / 0.05", 5.0, 0.05, 8), ("20 degrees / 0.2", 20.0, 0.2, 12), ("30 degrees / 0.3", 30.0, 0.3, 12)):
        start = A.offset_pose(r7, T_true, deg, tr, centre)
        pt = eng.align_to_map(t, codes, pts300, start[None], iterations=iters, **kw)
        pe = A.pose_error(pt["pose"][0], T_true)
        for eps, steps in ((1e-3, 64), (1e-4, 128)):
            r = eng.align_rays_to_map(t, codes, pts300, start[None], max_gap=MAX_GAP, raycast=dict(eps=eps, max_steps=steps), iterations=iters, **kw)
            e = A.pose_error(r["pose"][0], T_true)
            acc.append("| %s | %d | %g | %.2e / %.2e | %d | %.2e / %.2e | %d |" % (name, iters, eps, e[0], e[1], r["n_used"][0], pe[0], pe[1], pt["n_used"][0]))
            print(acc[-1], flush=True)

    # ---- time ----
    K = (140.0, 140.0, 79.5, 59.5)
    look = centre - T_true[:3, 3]
    z = look / np.sqrt((look * look).sum())
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.sqrt((x * x).sum())
    T_cam = A.rigid(np.stack([x, np.cross(z, x), z], 1), T_true[:3, 3])
    _, dirs_img, _ = M.pixel_rays(K, np.eye(4), 160, 120)
    shapes = [("450 rays x 8 hypotheses", pts_all[:450], T_true, 8)]
    shapes.append(("160 x 120 image x 1 hypothesis", observe(T_cam, dirs_img.astype(F64), background=9.0), T_cam, 1))
    tim = ["| shape | rows | cast ms | evaluation ms | evaluation - cast ms | call of 8 evaluations ms | per evaluation of the call ms | pairs | march rows | spread cast / evaluation |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for name, pts, T0, n_hyp in shapes:
        r8 = np.random.default_rng(n_hyp)
        c = (pts.astype(F64)[np.isfinite(pts).all(1)] @ T0[:3, :3].T + T0[:3, 3]).mean(0)
        hyp = np.stack([A.offset_pose(r8, T0, 2.0, 0.02, c) for _ in range(n_hyp)])
        rows = [AR.build(h, pts) for h in hyp]
        ow, dirv = np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows])
        f_cast = lambda: eng.cast_rays(t, codes, ow, dirv, normals=True, max_steps=64)
        f_eval = lambda: eng.align_rays_to_map(t, codes, pts, hyp, max_gap=MAX_GAP, raycast=dict(max_steps=64), iterations=1, **kw)
        f_call = lambda: eng.align_rays_to_map(t, codes, pts, hyp, max_gap=MAX_GAP, raycast=dict(max_steps=64), iterations=8, **kw)
        for f in (f_cast, f_eval, f_call):
            f()
        ts = {f: [] for f in (f_cast, f_eval, f_call)}
        for _ in range(args.reps):
            for f in (f_cast, f_eval, f_call):
                t0 = time.perf_counter()
                f()
                ts[f].append(time.perf_counter() - t0)
        med = {f: 1e3 * float(np.median(v)) for f, v in ts.items()}
        spread = {f: (max(v) - min(v)) / float(np.median(v)) for f, v in ts.items()}
        f_eval()
        st = eng.align_rays_stats()
        f_call()
        n_ev = max(1, eng.align_rays_stats()["evaluations"])
        tim.append("| %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %d | %d | %.0f %% / %.0f %% |" % (
            name, ow.shape[0], med[f_cast], med[f_eval], med[f_eval] - med[f_cast], med[f_call], med[f_call] / n_ev, st["pairs"], st["rows"],
            100 * spread[f_cast], 100 * spread[f_eval]))
        print(tim[-1], flush=True)
    text = ["## Accuracy on the device (300 rays, max_gap %.1f, observations cast at eps 1e-5)" % MAX_GAP, ""] + acc + [
        "", "## Time on the device (`python tools/measure_align_rays.py --reps %d`, fixture decoder `cars`, one MI355X)" % args.reps, ""] + tim + [""]
    print("\n".join(text))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text))
    eng.close()


if __name__ == "__main__":
    main()
