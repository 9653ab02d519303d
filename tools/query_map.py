#!/usr/bin/env python3
"""Ask a saved DSP-SLAM map (MapObjects.txt) about a batch of world points on the MI355X: which object each point belongs to, its signed
distance to that object's decoded surface (world units) and -- with --normals -- the surface's outward normal there, all objects and all
points in one call (dsp_map_query).

    python tools/query_map.py --config configs/config_kitti.json --map_dir map/kitti/07 --points sweep.npy [--normals] [--max_dist 0.1] --out query.npz

--points: an (n, 3) array of world-frame points (.npy).  --out receives obj (index into the map file's object order, -1 = inside no
object's unit sphere), id (the map's object id, -1 for none), dist (+inf for none), bound (distance to the nearest unit sphere the point is
outside of: dist <= bound certifies that obj is the nearest object) and, with --normals, normal.  With --max_dist D the file also holds the
association of points to objects: assoc_ids (the object ids that won a point with dist <= D, ascending), assoc_off (len + 1 offsets) and
assoc_pts (the point indices, grouped by object).
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
    ap.add_argument("--config", required=True)
    ap.add_argument("--map_dir", required=True)
    ap.add_argument("--points", required=True, metavar="FILE.npy", help="(n, 3) world-frame points")
    ap.add_argument("--normals", action="store_true", help="also return the winning surface's unit outward normal in the world frame")
    ap.add_argument("--max_dist", type=float, default=None, metavar="D", help="also write, per object id, the points it won with dist <= D")
    ap.add_argument("--out", required=True, metavar="FILE.npz")
    args = ap.parse_args()
    from reconstruct.utils import get_configs, get_decoder
    from dsp_slam_amd.map_objects import read_map_objects, query_points, associate
    cfg = get_configs(args.config)
    objs = read_map_objects(os.path.join(args.map_dir, "MapObjects.txt"))
    pts = np.asarray(np.load(args.points), np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        ap.error("--points must hold an (n, 3) array")
    eng = get_decoder(cfg).engine
    t0 = time.time()
    res = query_points(eng, objs, pts, normals=args.normals)
    st = eng.query_stats()
    print("queried %d points against %d objects in %.3f s: %d candidate rows in %d tiles (%.1f points per tile), %d chunks, %d passes" % (
        pts.shape[0], len(objs), time.time() - t0, st["rows"], st["tiles"], st["rows"] / max(1, st["tiles"]), st["chunks"], st["passes"]))
    hit = res["obj"] >= 0
    print("%d points inside an object's sphere, %d of them with dist <= bound (certified nearest), %d inside a shape" % (
        int(hit.sum()), int((hit & (res["dist"] <= res["bound"])).sum()), int((hit & (res["dist"] < 0)).sum())))
    out = {k: res[k] for k in ("obj", "id", "dist", "bound")}
    if args.normals:
        out["normal"] = res["normal"]
    if args.max_dist is not None:
        a = associate(res, args.max_dist)
        ids = sorted(a)
        out["assoc_ids"] = np.asarray(ids, np.int64)
        out["assoc_off"] = np.concatenate([[0], np.cumsum([a[i].shape[0] for i in ids])]).astype(np.int64)
        out["assoc_pts"] = np.concatenate([a[i] for i in ids]).astype(np.int64) if ids else np.zeros(0, np.int64)
        print("%d objects own %d points within %g" % (len(ids), int(out["assoc_off"][-1]), args.max_dist))
    np.savez(args.out, **out)


if __name__ == "__main__":
    main()
