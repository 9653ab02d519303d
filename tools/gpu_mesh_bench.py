#!/usr/bin/env python3
"""Mesh extraction on the MI355X: dense fp32 grid decode against the surface-band path (dsp_extract_meshes with the f16 prepass).

For the `cars` and `complex` fixture decoders at 32^3, 64^3 and 128^3 it times, per object:
  dense    dsp_extract_mesh without a prepass flag, one object per call (what MeshExtractor.extract_mesh_from_code does by default);
  band 1   dsp_extract_mesh with DSP_MESH_PREPASS_F16, one object per call;
  band 64  dsp_extract_meshes with DSP_MESH_PREPASS_F16 over 64 objects in one call (time / 64);
and prints the share of grid points that went through the fp32 kernel (surface band + audit) beside each band time.  Codes are
warm-start-sized (|z|inf 0.2-0.5, the magnitude a detection hands to the optimiser).  Every call returns to the host synchronised
(each ends with a stream synchronisation and the mesh copy), so the times are wall-clock per call, including the mesh fetch, after
warm-up, median of --reps repetitions.

    python tools/gpu_mesh_bench.py [--reps 5] [--dims 32 64 128] [--fixtures cars complex] [--out profiles/mesh_band_run.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def codes_of(name, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        if name == "complex":
            c = rng.normal(0.0, 0.1, 64)
        else:
            c = rng.normal(0.0, 0.02, 64)
            c[:3] = rng.uniform((0.15, -0.35, -0.1), (0.4, 0.0, 0.2))
        out.append(c.astype(np.float32))
    return out


def timed(fn, reps):
    fn()                                   # warm-up (buffers grown, tables built)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--fixtures", nargs="+", default=["cars", "complex"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the table (markdown) here")
    args = ap.parse_args()
    from dsp_slam_amd import fixtures, engine as E
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    rows = []
    for name in args.fixtures:
        sd = fixtures.load_decoder_npz(fixtures.fixture_path(name))
        specs = fixtures.fixture_specs(name)
        net = specs["NetworkSpecs"]
        layers = fold_weight_norm(sd, len(net["dims"]) + 1)
        code_len = specs.get("CodeLength", 64)
        eng = E.Engine(layers, net["latent_in"], code_len, device=0)
        codes = codes_of(name, args.batch, 1)
        for n in args.dims:
            one = codes[0]
            reps = args.reps if n < 128 else max(2, args.reps // 2)
            t_dense = timed(lambda: eng.extract_mesh(one, n), reps)
            t_band1 = timed(lambda: eng.extract_mesh(one, n, prepass="f16"), reps)
            st1 = eng.mesh_stats()
            t_bandb = timed(lambda: eng.extract_meshes(codes, n, prepass="f16"), reps) / len(codes)
            stb = eng.mesh_stats()
            frac1 = (st1["band_points"] + st1["audit_points"] + st1["dense_points"]) / max(1, st1["prepass_points"])
            fracb = (stb["band_points"] + stb["audit_points"] + stb["dense_points"]) / max(1, stb["prepass_points"])
            row = (name, n, 1e3 * t_dense, 1e3 * t_band1, frac1, 1e3 * t_bandb, fracb, stb["reruns"])
            rows.append(row)
            print("%-8s %4d^3  dense %8.3f ms | band 1 %8.3f ms (fp32 %.3f) | band x%d %8.3f ms/obj (fp32 %.3f, re-runs %d)" % (
                row[0], row[1], row[2], row[3], row[4], len(codes), row[5], row[6], row[7]), flush=True)
        eng.close()
    lines = ["| decoder | grid | dense ms/obj | band 1 ms/obj | fp32 share | band x%d ms/obj | fp32 share | re-runs | dense / band 1 | dense / band x%d |" % (args.batch, args.batch),
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d^3 | %.3f | %.3f | %.3f | %.3f | %.3f | %d | %.2f | %.2f |" % (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7],
                                                                                           r[2] / r[3], r[2] / r[5]))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
