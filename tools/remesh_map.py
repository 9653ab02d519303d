#!/usr/bin/env python3
"""Batch re-decode every object of a saved DSP-SLAM map (MapObjects.txt) on the MI355X: one kernel launch decodes the
D^3 SDF grid of ALL objects (saved as <id>_sdf.npy); marching cubes then runs on the device on each decoded grid and the mesh is
written as <id>.ply next to the pose <id>.npy -- the files the reference's extract_map_objects.py:46-63 produces.

    python tools/remesh_map.py --config configs/config_kitti.json --map_dir map/kitti/07 [--voxels_dim 64] [--prepass f16]

--prepass f16|bf16 meshes the whole map in one batched call instead (dsp_extract_meshes: low-precision prepass over the grids, fp32
only in the surface band; the same meshes, bit for bit) and writes no <id>_sdf.npy, since those volumes are not fp32 away from the
surface.

--refine STEPS (default 0 = off: the files above, unchanged) meshes the whole map in one batched call and projects every vertex onto the
decoder's zero set with STEPS capped Newton steps on the device (dsp_meshes_refine); <id>.ply then holds the refined vertices with the
decoder's own unit normals (nx, ny, nz).  With --posterior FILE.npz (what tools/reoptimise_map.py --posterior writes) every vertex also
carries `quality` = sigma, the standard deviation of the surface along its normal under that object's code variance; an object without a
usable record (no observation, singular system) and every frozen code entry count as variance 0.  No <id>_sdf.npy is written.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsp_slam_amd"))
sys.path.insert(0, ROOT)


def code_variances(post, ids, code_len):
    """(n, code_len) code variances for the map's objects from a posterior file (ids, status, var_code): the row of the object's id when its
    record is usable (status 0), else zeros; a frozen code entry is stored as 0 (include/dsp_gn.h) and anything not finite or negative is
    taken as 0 too."""
    var = np.zeros((len(ids), code_len))
    row = {int(i): k for k, i in enumerate(post["ids"])}
    for k, i in enumerate(ids):
        j = row.get(int(i))
        if j is None or int(post["status"][j]) != 0:
            continue
        v = np.asarray(post["var_code"][j], np.float64)[:code_len]
        var[k, :v.shape[0]] = np.where(np.isfinite(v) & (v > 0), v, 0.0)
    return var


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--map_dir", required=True)
    ap.add_argument("--voxels_dim", type=int, default=64)
    ap.add_argument("--prepass", choices=("off", "f16", "bf16"), default="off",
                    help="off (default): decode every grid in fp32, save it as <id>_sdf.npy, mesh it.  f16 / bf16: mesh all objects in one "
                         "batched call with the low-precision prepass (fp32 only in the surface band; identical meshes); no <id>_sdf.npy is "
                         "written, because those volumes are not fp32 away from the surface")
    ap.add_argument("--refine", type=int, default=0, metavar="STEPS",
                    help="0 (default): off.  1..8: project every vertex onto the decoder's zero set with STEPS Newton steps and write the refined "
                         "vertices with analytic normals")
    ap.add_argument("--posterior", default=None, metavar="FILE.npz",
                    help="with --refine: the file reoptimise_map.py --posterior wrote; each vertex gets quality = sigma from its object's code variance")
    args = ap.parse_args()
    if args.posterior is not None and not args.refine:
        ap.error("--posterior needs --refine")
    from reconstruct.utils import get_configs, get_decoder, write_mesh_to_ply, write_mesh_to_ply_with_normals, convert_sdf_voxels_to_mesh
    from reconstruct.optimizer import MeshExtractor
    from dsp_slam_amd.map_objects import read_map_objects
    cfg = get_configs(args.config)
    objs = read_map_objects(os.path.join(args.map_dir, "MapObjects.txt"))
    save_dir = os.path.join(args.map_dir, "objects")
    if args.refine:
        ext = MeshExtractor(get_decoder(cfg), cfg.optimizer.code_len, args.voxels_dim, prepass=None if args.prepass == "off" else args.prepass)
        var = None
        if args.posterior is not None:
            var = code_variances(dict(np.load(args.posterior)), [o["id"] for o in objs], cfg.optimizer.code_len)
        t0 = time.time()
        meshes = ext.extract_refined_meshes_from_codes([o["code"] for o in objs], steps=args.refine, var_codes=var)
        print("meshed and refined %d grids of %d^3 (%d steps) in %.3f s" % (len(objs), args.voxels_dim, args.refine, time.time() - t0))
        os.makedirs(save_dir, exist_ok=True)
        n_ok = 0
        for o, m in zip(objs, meshes):
            np.save(os.path.join(save_dir, "%d.npy" % o["id"]), o["pose"])
            if m.vertices.shape[0] == 0:
                print("object %d: Surface level must be within volume data range." % o["id"])
                continue
            write_mesh_to_ply_with_normals(m.vertices, m.normals, m.faces, os.path.join(save_dir, "%d.ply" % o["id"]),
                                           quality=m.sigma if var is not None else None)
            n_ok += 1
        print("wrote %d meshes, largest |sdf| at a vertex %.3g" % (n_ok, max([float(np.abs(m.sdf).max()) for m in meshes if m.sdf.shape[0]] + [0.0])))
        return
    if args.prepass != "off":
        ext = MeshExtractor(get_decoder(cfg), cfg.optimizer.code_len, args.voxels_dim, prepass=args.prepass)
        t0 = time.time()
        meshes = ext.extract_meshes_from_codes([o["code"] for o in objs])
        st = ext.decoder.engine.mesh_stats()
        print("meshed %d grids of %d^3 in %.3f s (%s prepass: %.2f %% of the grid points in fp32, %d objects re-run in fp32)" % (
            len(objs), args.voxels_dim, time.time() - t0, args.prepass,
            100.0 * (st["band_points"] + st["audit_points"] + st["dense_points"]) / max(1, st["prepass_points"]), st["reruns"]))
        os.makedirs(save_dir, exist_ok=True)
        n_ok = 0
        for o, m in zip(objs, meshes):
            np.save(os.path.join(save_dir, "%d.npy" % o["id"]), o["pose"])
            if m.vertices.shape[0] == 0:
                print("object %d: Surface level must be within volume data range." % o["id"])
                continue
            write_mesh_to_ply(m.vertices, m.faces, os.path.join(save_dir, "%d.ply" % o["id"]))
            n_ok += 1
        print("wrote %d meshes" % n_ok)
        return
    ext = MeshExtractor(get_decoder(cfg), cfg.optimizer.code_len, args.voxels_dim)
    t0 = time.time()
    grids = ext.decode_grids([o["code"] for o in objs])
    print("decoded %d grids of %d^3 in %.3f s" % (len(objs), args.voxels_dim, time.time() - t0))
    os.makedirs(save_dir, exist_ok=True)
    for o, g in zip(objs, grids):
        np.save(os.path.join(save_dir, "%d.npy" % o["id"]), o["pose"])
        np.save(os.path.join(save_dir, "%d_sdf.npy" % o["id"]), g)
    t0 = time.time()
    n_ok = 0
    for o, g in zip(objs, grids):
        try:
            vertices, faces = convert_sdf_voxels_to_mesh(g)      # marching cubes on the grid decoded above: no second decode
        except ValueError as e:          # no zero crossing inside the grid
            print("object %d: %s" % (o["id"], e))
            continue
        write_mesh_to_ply(vertices, faces, os.path.join(save_dir, "%d.ply" % o["id"]))
        n_ok += 1
    print("meshed %d objects in %.3f s" % (n_ok, time.time() - t0))


if __name__ == "__main__":
    main()
