#!/usr/bin/env python3
"""Render a saved DSP-SLAM map (MapObjects.txt) from a pinhole camera on the MI355X without meshing it: per pixel the z-depth of the first
object surface, the object it belongs to and -- with --normals -- its world normal, all objects and all pixels in one call
(dsp_map_raycast).

    python tools/render_map.py --map map/kitti/07/MapObjects.txt --decoder weights/deepsdf/cars_64 --intrinsics 718.856 718.856 607.19 185.22 \
        --size 1241 376 --pose t_world_cam.npy [--normals] [--eps 1e-3 --relax 1 --max-steps 64 --t-max 80] --out render.npz

--decoder: a DeepSDF experiment directory (specs.json, ModelParameters/latest.pth).  --pose: a (4, 4) rigid camera-to-world matrix (.npy).
Integer pixel coordinates are pixel centres: the pixel in column j, row i looks along ((j - cx) / fx, (i - cy) / fy, 1).  --out receives
(H, W) images: depth (+inf where nothing is hit), id (the map's object id, -1 for none), obj (index into the map file's object order),
status (0 miss, 1 hit, 2 undecided: raise --max-steps), t, dist and, with --normals, normal (H, W, 3).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsp_slam_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", required=True, metavar="MapObjects.txt")
    ap.add_argument("--decoder", required=True, metavar="DIR", help="DeepSDF experiment directory")
    ap.add_argument("--intrinsics", required=True, type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--size", required=True, type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--pose", required=True, metavar="FILE.npy", help="(4, 4) camera-to-world")
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--eps", type=float, default=None)
    ap.add_argument("--relax", type=float, default=None)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--t-max", type=float, default=None)
    ap.add_argument("--out", required=True, metavar="FILE.npz")
    args = ap.parse_args()
    from deep_sdf.workspace import config_decoder
    from dsp_slam_amd.map_objects import read_map_objects, render
    objs = read_map_objects(args.map)
    pose = np.asarray(np.load(args.pose), np.float64)
    if pose.shape != (4, 4):
        ap.error("--pose must hold a (4, 4) matrix")
    params = {k: v for k, v in (("eps", args.eps), ("relax", args.relax), ("max_steps", args.max_steps), ("t_max", args.t_max)) if v is not None}
    eng = config_decoder(args.decoder).engine
    w, h = args.size
    t0 = time.time()
    img = render(eng, objs, args.intrinsics, pose, w, h, normals=args.normals, **params)
    st = eng.raycast_stats()
    print("rendered %d x %d pixels of %d objects in %.3f s: %d pairs, %d decoder rows in %d tiles, %d rounds, %d passes" % (
        w, h, len(objs), time.time() - t0, st["pairs"], st["rows"], st["tiles"], st["rounds"], st["passes"]))
    print("%d pixels hit, %d undecided (%d pairs exhausted)" % (int((img["obj"] >= 0).sum()), int((img["status"] == 2).sum()), st["exhausted"]))
    out = {k: img[k] for k in ("depth", "id", "obj", "status", "t", "dist")}
    if args.normals:
        out["normal"] = img["normal"]
    np.savez(args.out, **out)


if __name__ == "__main__":
    main()
