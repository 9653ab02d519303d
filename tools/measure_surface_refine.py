#!/usr/bin/env python3
"""What projecting the mesh vertices onto the decoder's zero set costs and buys (dsp_meshes_refine), on one MI355X:

    python tools/measure_surface_refine.py [--dims 32 64] [--batch 8] [--reps 5] [--out profiles/table.md]

For each fixture decoder and grid size: the batched extraction's own time (dsp_extract_meshes + dsp_meshes_fetch), then per step count
the time of dsp_meshes_refine + dsp_meshes_fetch_attributes on that extraction (median of --reps, wall clock around the calls) and the
largest |sdf| at the vertices as the device evaluates it -- steps 0 is the marching-cubes mesh as it is today.  Times are per call for
--batch objects.  First measurements: recorded, nothing is gated on them.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_COUNTS = (0, 1, 2, 4, 6, 8)


def median_time(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--fixtures", nargs="+", default=["cars", "chairs32", "complex"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the table (markdown) here")
    args = ap.parse_args()
    from dsp_slam_amd import fixtures, engine as E, _lib as L
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    lib = L.load()
    lines = ["| decoder | grid | objects | vertices | extraction ms | steps | refine + fetch ms | max abs sdf at the vertices |", "|---|---|---|---|---|---|---|---|"]
    for name in args.fixtures:
        specs = fixtures.fixture_specs(name)
        net = specs["NetworkSpecs"]
        layers = fold_weight_norm(fixtures.load_decoder_npz(fixtures.fixture_path(name)), len(net["dims"]) + 1)
        code_len = specs.get("CodeLength", 64)
        eng = E.Engine(layers, net["latent_in"], code_len, device=0)
        rng = np.random.default_rng(5)
        codes = [np.zeros(code_len, np.float32)] + [rng.uniform(-0.3, 0.3, code_len).astype(np.float32) for _ in range(args.batch - 1)]
        c64 = np.stack([L.code64(c) for c in codes])
        var = np.full((len(codes), L.CODE_LEN), 1e-3)
        for n in args.dims:
            t_ext = median_time(lambda: eng.extract_meshes(codes, n), args.reps)
            nv, nf = np.zeros(len(codes), np.int64), np.zeros(len(codes), np.int64)
            L.check(lib.dsp_extract_meshes(eng._h, L.ptr(c64), len(codes), n, 0, 0.0, L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p)), eng._h, "dsp_extract_meshes")
            tv = int(nv.sum())
            verts, nrm, sdf, sig = np.zeros((tv, 3), np.float32), np.zeros((tv, 3), np.float32), np.zeros(tv, np.float32), np.zeros(tv, np.float32)

            def refine(steps, with_var):
                v = L.ptr(var, L.c_f64p) if with_var else None
                L.check(lib.dsp_meshes_refine(eng._h, len(codes), L.ptr(nv, L.c_i64p), steps, 0.0, v), eng._h, "dsp_meshes_refine")
                L.check(lib.dsp_meshes_fetch_attributes(eng._h, len(codes), L.ptr(nv, L.c_i64p), L.ptr(verts), L.ptr(nrm), L.ptr(sdf),
                                                        L.ptr(sig) if with_var else None), eng._h, "dsp_meshes_fetch_attributes")

            for steps in STEP_COUNTS:
                t = median_time(lambda: refine(steps, False), args.reps)
                lines.append("| %s | %d^3 | %d | %d | %.2f | %d | %.2f | %.2e |" % (name, n, len(codes), tv, 1e3 * t_ext, steps, 1e3 * t, float(np.abs(sdf).max())))
            t = median_time(lambda: refine(6, True), args.reps)
            lines.append("| %s | %d^3 | %d | %d | %.2f | 6 + sigma | %.2f | %.2e |" % (name, n, len(codes), tv, 1e3 * t_ext, 1e3 * t, float(np.abs(sdf).max())))
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
