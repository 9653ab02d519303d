#!/usr/bin/env python3
"""How far the fp32 restatement of the observation report sits from its fp64 twin, on the inputs of tests/test_gpu_report.py.

    python tools/measure_report.py --measure [out.json]

For every member of tests/report_ref.py's joint objects (num_depth_samples 50 and 64) and multi-view objects (50), at the state the fp32
oracle returns after report_ref.N_IT iterations, the report is evaluated twice -- report_ref.evaluate32 (unmodified oracle pieces, float32)
and report_ref.evaluate64 (oracle.dsp_oracle._decode64, float64, on the same in-sphere set) -- and the worst |fp32 - fp64| per float field
is printed: the TAU_* of tests/report_ref.py and the table of profiles/report.md.  It also prints, per case, the share of rays whose band or
kept decisions differ between fp32, its sdf_jitter = +-2e-7 twins and fp64 (the rays the GPU test leaves out of its count comparison;
the cap is 0.5 % per case), so that the seeds are checked here, on the CPU.  CPU only; reads nothing outside the repository.

    python tools/measure_report.py --time RUNS [--objects 64]      # needs an MI355X

times the headline batch (bench.py's cfg2x64) with the report off and on: the "added time of the pass" of profiles/report.md.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import dsp_oracle as O  # noqa: E402
from dsp_slam_amd import fixtures  # noqa: E402
import multiview_oracle as MV  # noqa: E402
import report_ref as R  # noqa: E402

FIELDS = ("pt_sdf", "ray_depth", "ray_hit", "ray_residual", "sum_s", "sum_r")


def members():
    """-> (case, decoder, prm, (pts, rays, depth), (t_obj_cam, code, depths)) per evaluated member."""
    dec = O.fold_decoder(fixtures.load_decoder_npz(fixtures.fixture_path("cars")), fixtures.SPECS)
    for n_depth in (50, 64):
        prm = R.oracle_params(n_depth)
        for i, o in enumerate(R.joint_objects()):
            res = O.reconstruct_object(dec, prm, o["t_cam_obj_init"], o["pts"], o["rays"], o["depth"])
            if not res["is_good"]:
                continue
            t_oc = O._inv(res["t_cam_obj"])
            yield ("joint D=%d" % n_depth, dec, prm, (o["pts"], o["rays"], o["depth"]), (t_oc, res["code"], R.derived_depths(t_oc, n_depth)))
    prm = R.oracle_params(50)
    for o in R.multiview_objects():
        res = MV.reconstruct_object_multiview(dec, prm, o["t_cam_obj_init"], o["views"])
        t_oc = O._inv(res["t_cam_obj"])
        for v in o["views"]:
            t_v, d = MV.view_state(t_oc, v["t_ref_cam"], 50)
            yield ("multi-view D=50", dec, prm, (v["pts"], v["rays"], v["depth"]), (t_v, res["code"], d))


def measure():
    worst = {f: 0.0 for f in FIELDS}
    cases = {}
    for case, dec, prm, (pts, rays, depth), (t_oc, code, depths) in members():
        r32 = R.evaluate32(dec, prm, pts, rays, depth, t_oc, code, depths)
        r64 = R.evaluate64(dec, prm, pts, rays, depth, t_oc, code, depths, r32["in_mask"])
        c = cases.setdefault(case, dict(rays=0, excluded=0, **{f: 0.0 for f in FIELDS}))
        evaluated = r32["V"] >= 10
        for f in FIELDS:
            if f.startswith("ray_") or f == "sum_r":
                if not evaluated or rays.shape[0] == 0:
                    continue
            a, b = np.asarray(r32[f], np.float64), np.asarray(r64[f], np.float64)
            if f == "sum_r":          # fp64 on the fp32 evaluation's kept set: the reference the GPU test holds every member to
                b = np.asarray(R.sum_r64_on(r64, r32["ray_counts"][:, 2], prm.b1))
            if a.size:
                c[f] = max(c[f], float(np.abs(a - b).max()))
                worst[f] = max(worst[f], c[f])
        if evaluated and rays.shape[0]:
            ok = R.agreeing_rays(dec, prm, pts, rays, depth, t_oc, code, depths, r32, r64)
            c["rays"] += int(ok.shape[0])
            c["excluded"] += int((~ok).sum())
    return worst, cases


def time_pass(runs, objects):
    """MI355X: the device time of a run of the headline batch (bench.py's cfg2x64: `objects` objects of 2000 surface points + 500
    free-space rays, 10 iterations) with the report off -- the launches of a library without the feature -- and on, interleaved, `runs`
    timed runs each after one warm-up run each; dsp_stats.ms_total (HIP events around the run on the handle's stream)."""
    from dsp_slam_amd import engine as E, synth
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    sd = fixtures.load_decoder_npz(fixtures.fixture_path("cars"))
    layers = fold_weight_norm(sd, len(fixtures.SPECS["NetworkSpecs"]["dims"]) + 1)
    eng = E.Engine(layers, fixtures.SPECS["NetworkSpecs"]["latent_in"], fixtures.SPECS["CodeLength"], device=0)
    objs = synth.make_batch(objects, first_seed=1, n_surface=2000, n_background=500)
    b = eng.batch(E.gn_params(), [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs])
    ms = {0: [], 1: []}
    for i in range(2 * (runs + 1)):
        on = i % 2
        b.set_report(bool(on))
        b.run()
        if i >= 2:
            ms[on].append(b.stats()["ms_total"])
    rep = b.report()
    b.close()
    eng.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print("headline batch, %d objects, %d timed runs each: report off %.3f ms (min %.3f, max %.3f), on %.3f ms (min %.3f, max %.3f): + %.3f ms = + %.2f %%" % (
        objects, runs, med[0], min(ms[0]), max(ms[0]), med[1], min(ms[1]), max(ms[1]), med[1] - med[0], 100.0 * (med[1] - med[0]) / med[0]))
    print("report: %d points, %d rays, %d good members" % (rep["pt_sdf"].shape[0], rep["ray_depth"].shape[0], int((rep["status"] == 0).sum())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", nargs="?", const="-", default=None, metavar="OUT.json")
    ap.add_argument("--time", type=int, default=0, metavar="RUNS", help="needs an MI355X: time the headline batch with the report off and on")
    ap.add_argument("--objects", type=int, default=64)
    args = ap.parse_args()
    if args.time > 0:
        time_pass(args.time, args.objects)
        return
    if args.measure is None:
        ap.error("nothing to do: pass --measure or --time RUNS")
    worst, cases = measure()
    for case, c in cases.items():
        print("%-16s %s | rays %d, excluded %d (%.2f %%)" % (case, "  ".join("%s %.2e" % (f, c[f]) for f in FIELDS), c["rays"], c["excluded"],
                                                             100.0 * c["excluded"] / max(c["rays"], 1)))
    for f in FIELDS:          # rounded UP to two significant digits: the constants of tests/report_ref.py
        e = 10.0 ** (np.floor(np.log10(worst[f])) - 1)
        print("TAU_%s = %.1e   (worst %.3e)" % (f.upper(), np.ceil(worst[f] / e) * e, worst[f]))
    if args.measure != "-":
        with open(args.measure, "w") as fh:
            json.dump(dict(tau=worst, cases=cases), fh, indent=1)


if __name__ == "__main__":
    main()
