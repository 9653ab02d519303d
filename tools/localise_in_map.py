#!/usr/bin/env python3
"""Locate a sensor in a saved DSP-SLAM map (MapObjects.txt) from a cloud of points in the sensor's frame, on the MI355X: batched SE(3)
Gauss-Newton against the objects' decoded surfaces, one run per initial pose, all in one call (dsp_map_align).

    python tools/localise_in_map.py --map MapObjects.txt --decoder DIR --points FILE.npy --init FILE.npy [--weights FILE.npy]
                                    [--iterations N] [--max-dist D] [--huber H] [--step-control L0 UP DOWN LMIN LMAX]
                                    [--rays [--origins FILE.npy] [--max-gap G]] --out FILE.npz

--decoder: the DeepSDF experiment directory (specs.json and the model parameters).  --points: (n, 3) sensor-frame points.  --init: one
(4, 4) or several (k, 4, 4) initial sensor-to-world poses -- a relocaliser's seeds; they are refined independently and `best` names the
one with the lowest cost among those that kept support.  --out receives pose (k, 4, 4), status (0 iterations ran out, 1 converged, 2 no
support, 3 singular), cost, cost0, n_used, evaluations, steps, information (k, 6, 6: the Gauss-Newton matrix of [v, omega] at the returned
pose), best, and per hypothesis and point obj, id (the map's object id, -1 for none) and dist at the returned pose.

--rays: the points are the measured END POINTS of depth rays from the sensor origin (--origins: (n, 3) sensor-frame origins instead), and
the pose is found by projective Gauss-Newton against the ray-cast map (dsp_map_align_rays): occlusion between objects and free space count,
and points of the background need not be cut away first -- the gate --max-gap on |measured depth - cast depth| (default 2 x max-dist, inf
for none) leaves them out.  --out then also receives t (the cast depth along each ray) and status_ray (0 miss, 1 hit, 2 undecided).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsp_slam_amd"))
sys.path.insert(0, ROOT)

STATUS = {0: "iterations ran out", 1: "converged", 2: "no support", 3: "singular"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", required=True, metavar="MapObjects.txt")
    ap.add_argument("--decoder", required=True, metavar="DIR", help="DeepSDF experiment directory")
    ap.add_argument("--points", required=True, metavar="FILE.npy", help="(n, 3) sensor-frame points")
    ap.add_argument("--init", required=True, metavar="FILE.npy", help="(4, 4) or (k, 4, 4) initial sensor-to-world poses")
    ap.add_argument("--weights", default=None, metavar="FILE.npy", help="(n,) weights >= 0")
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--max-dist", type=float, default=None, metavar="D", help="gate on |distance|, world units")
    ap.add_argument("--huber", type=float, default=None, metavar="H")
    ap.add_argument("--step-control", type=float, nargs=5, default=None, metavar=("L0", "UP", "DOWN", "LMIN", "LMAX"),
                    help="Levenberg-Marquardt step control (default: off, plain Gauss-Newton)")
    ap.add_argument("--rays", action="store_true", help="align the points as depth rays against the ray-cast map")
    ap.add_argument("--origins", default=None, metavar="FILE.npy", help="with --rays: (n, 3) sensor-frame ray origins (default: the sensor origin)")
    ap.add_argument("--max-gap", type=float, default=None, metavar="G", help="with --rays: gate on |measured depth - cast depth|")
    ap.add_argument("--out", required=True, metavar="FILE.npz")
    args = ap.parse_args()
    from deep_sdf.workspace import config_decoder
    from dsp_slam_amd.map_objects import read_map_objects, localise, localise_rays
    if not args.rays and (args.origins is not None or args.max_gap is not None):
        ap.error("--origins and --max-gap go with --rays")
    objs = read_map_objects(args.map)
    pts = np.asarray(np.load(args.points), np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        ap.error("--points must hold an (n, 3) array")
    init = np.asarray(np.load(args.init), np.float64)
    if init.shape[-2:] != (4, 4):
        ap.error("--init must hold one (4, 4) pose or (k, 4, 4) poses")
    init = init.reshape(-1, 4, 4)
    weights = None if args.weights is None else np.asarray(np.load(args.weights), np.float32).reshape(-1)
    params = {k: v for k, v in (("iterations", args.iterations), ("max_dist", args.max_dist), ("huber", args.huber),
                                ("step_control", args.step_control)) if v is not None}
    eng = config_decoder(args.decoder).engine
    t0 = time.time()
    keys = ("pose", "status", "cost", "cost0", "n_used", "evaluations", "steps", "information", "obj", "id", "dist")
    if args.rays:
        origins = None if args.origins is None else np.asarray(np.load(args.origins), np.float32).reshape(-1, 3)
        if args.max_gap is not None:
            params["max_gap"] = args.max_gap
        res = localise_rays(eng, objs, pts, init, origins=origins, weights=weights, **params)
        st = eng.align_rays_stats()
        keys += ("t", "status_ray")
        print("aligned %d rays to %d objects from %d initial poses in %.3f s: %d evaluations, %d (ray, object) pairs, %d march rows in %d tiles" % (
            pts.shape[0], len(objs), init.shape[0], time.time() - t0, st["evaluations"], st["pairs"], st["rows"], st["tiles"]))
    else:
        res = localise(eng, objs, pts, init, weights=weights, **params)
        st = eng.align_stats()
        print("aligned %d points to %d objects from %d initial poses in %.3f s: %d evaluations, %d candidate rows in %d tiles" % (
            pts.shape[0], len(objs), init.shape[0], time.time() - t0, st["evaluations"], st["rows"], st["tiles"]))
    for k in range(init.shape[0]):
        print("  pose %d: %s after %d evaluations, cost %.3e (from %.3e), %d of %d points used%s" % (
            k, STATUS[int(res["status"][k])], res["evaluations"][k], res["cost"][k], res["cost0"][k], res["n_used"][k], pts.shape[0],
            "  <- best" if k == res["best"] else ""))
    np.savez(args.out, **{k: res[k] for k in keys}, best=np.int64(res["best"]))


if __name__ == "__main__":
    main()
