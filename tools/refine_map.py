#!/usr/bin/env python3
"""Move the objects of a saved DSP-SLAM map (MapObjects.txt) to where depth images from KNOWN camera poses say they are, on the MI355X: one
SE(3) correction per object, projective Gauss-Newton against the ray-cast map (dsp_map_align_objects).  With --shapes the objects' shape
codes are refitted to the same rays instead (dsp_map_align_shapes), and with --with-pose their poses with them.

    python tools/refine_map.py --map MapObjects.txt --decoder DIR --intrinsics FX FY CX CY --depth FILE.npy [FILE.npy ...]
                               --pose FILE.npy [FILE.npy ...] [--only ID,ID] [--iterations N] [--max-dist D] [--huber H]
                               [--step-control L0 UP DOWN LMIN LMAX] [--max-gap G] --out MapObjects.txt [--report FILE.npz]
                               [--shapes [--with-pose] [--code-reg K] [--code-anchor K]]

--decoder: the DeepSDF experiment directory (specs.json and the model parameters).  --depth: one (height, width) z-depth image per frame
(pixels whose depth is not finite or not positive are skipped); --pose: the (4, 4) camera-to-world pose of each frame, in the same order.
Pixel convention: map_objects.pixel_rays.  --only: the ids to refine; the other objects keep their pose and still occlude.  --max-gap: the
gate on |measured depth - cast depth| (default 2 x max-dist, inf for none): pixels of the background need not be cut away first.
--out receives the map with the corrected poses (scales and codes unchanged).  --report receives per object id, status (0 iterations ran
out, 1 converged, 2 no support, 3 singular), evaluations, steps, cost, cost0, n_used, correction (4, 4), information (6, 6: the
Gauss-Newton matrix of the correction's left perturbation [v, omega]), and per ray frame, pixel, obj, id, dist, t, status_ray.
--shapes: refit the codes (poses fixed unless --with-pose); --code-reg K weighs |z|^2, --code-anchor K weighs |z - z_input|^2 (both 0 by
default); step control defaults to ON here (1e-3 10 0.1 1e-9 1e9: plain Gauss-Newton on the code is not monotone), "--step-control 0 0 0
0 0" turns it off.  --out then receives the refitted codes as well, and the report's information is 70 x 70 ([v, omega, dz]) with `codes`.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsp_slam_amd"))
sys.path.insert(0, ROOT)

SHAPES_STEP_CONTROL = (1e-3, 10.0, 0.1, 1e-9, 1e9)
STATUS = {0: "iterations ran out", 1: "converged", 2: "no support", 3: "singular"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", required=True, metavar="MapObjects.txt")
    ap.add_argument("--decoder", required=True, metavar="DIR", help="DeepSDF experiment directory")
    ap.add_argument("--intrinsics", required=True, type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--depth", required=True, nargs="+", metavar="FILE.npy", help="(height, width) z-depth images")
    ap.add_argument("--pose", required=True, nargs="+", metavar="FILE.npy", help="(4, 4) camera-to-world poses, one per depth image")
    ap.add_argument("--only", default=None, metavar="ID,ID", help="refine these object ids only")
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--max-dist", type=float, default=None, metavar="D", help="gate on |distance|, world units")
    ap.add_argument("--huber", type=float, default=None, metavar="H")
    ap.add_argument("--step-control", type=float, nargs=5, default=None, metavar=("L0", "UP", "DOWN", "LMIN", "LMAX"),
                    help="Levenberg-Marquardt step control (default: off, plain Gauss-Newton)")
    ap.add_argument("--max-gap", type=float, default=None, metavar="G", help="gate on |measured depth - cast depth|")
    ap.add_argument("--shapes", action="store_true", help="refit the objects' shape codes (dsp_map_align_shapes)")
    ap.add_argument("--with-pose", action="store_true", help="with --shapes: solve for the poses as well")
    ap.add_argument("--code-reg", type=float, default=None, metavar="K", help="with --shapes: weight of |z|^2")
    ap.add_argument("--code-anchor", type=float, default=None, metavar="K", help="with --shapes: weight of |z - z_input|^2")
    ap.add_argument("--out", required=True, metavar="MapObjects.txt")
    ap.add_argument("--report", default=None, metavar="FILE.npz")
    args = ap.parse_args()
    from deep_sdf.workspace import config_decoder
    from dsp_slam_amd.map_objects import read_map_objects, write_map_objects, refine_poses_depth, refine_shapes_depth
    if not args.shapes and (args.with_pose or args.code_reg is not None or args.code_anchor is not None):
        ap.error("--with-pose, --code-reg and --code-anchor belong to --shapes")
    if len(args.depth) != len(args.pose):
        ap.error("one --pose per --depth")
    objs = read_map_objects(args.map)
    depth = [np.asarray(np.load(f), np.float32) for f in args.depth]
    poses = [np.asarray(np.load(f), np.float64) for f in args.pose]
    if any(d.ndim != 2 for d in depth) or any(p.shape != (4, 4) for p in poses):
        ap.error("--depth holds (height, width) images, --pose (4, 4) poses")
    only = None if args.only is None else [int(x) for x in args.only.split(",") if x.strip()]
    params = {k: v for k, v in (("iterations", args.iterations), ("max_dist", args.max_dist), ("huber", args.huber), ("step_control", args.step_control),
                                ("max_gap", args.max_gap)) if v is not None}
    eng = config_decoder(args.decoder).engine
    t0 = time.time()
    if args.shapes:
        params.setdefault("step_control", SHAPES_STEP_CONTROL)
        params.update({k: v for k, v in (("code_reg", args.code_reg), ("code_anchor", args.code_anchor)) if v is not None})
        res, moved = refine_shapes_depth(eng, objs, depth, args.intrinsics, poses, only=only, unknowns="pose+code" if args.with_pose else "code", **params)
        st = eng.align_shapes_stats()
    else:
        res, moved = refine_poses_depth(eng, objs, depth, args.intrinsics, poses, only=only, **params)
        st = eng.align_objects_stats()
    print("refined %d objects against %d rays of %d frames in %.3f s: %d evaluations, %d (ray, object) pairs, %d march rows in %d tiles" % (
        len(objs), res["pixel"].shape[0], len(depth), time.time() - t0, st["evaluations"], st["pairs"], st["rows"], st["tiles"]))
    for k, o in enumerate(objs):
        step = np.asarray(moved[k]["pose"], np.float64)[:3, 3] - np.asarray(o["pose"], np.float64)[:3, 3]
        print("  object %d: %s after %d evaluations, cost %.3e (from %.3e), %d rays used, centre moved %.4f" % (
            o["id"], "not refined" if only is not None and o["id"] not in only else STATUS[int(res["status"][k])], res["evaluations"][k], res["cost"][k],
            res["cost0"][k], res["n_used"][k], float(np.sqrt((step * step).sum()))))
    write_map_objects(args.out, moved)
    if args.report:
        keys = ("status", "evaluations", "steps", "cost", "cost0", "n_used", "correction", "information", "frame", "pixel", "obj", "id", "dist", "t",
                "status_ray") + (("codes",) if args.shapes else ())
        np.savez(args.report, object_id=np.array([o["id"] for o in objs], np.int64), **{k: res[k] for k in keys})


if __name__ == "__main__":
    main()
