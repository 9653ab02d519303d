#!/usr/bin/env python3
"""What the mask of unknowns (dsp_batch_unknowns) costs and what it is good for (needs an MI355X); writes the markdown of profiles/unknowns.md.

    python tools/measure_unknowns.py [--parent DIR] [--rounds 3] [--runs 9] [--objects 64] [--test-log FILE] [--out profiles/unknowns.md]

1. Cost with the mask OFF, parent commit against this tree (--parent DIR: a checkout of the parent commit with its library built; skipped
   without it).  Two figures, each from a fresh process per run, the trees alternating P N P N ...: bench.py's headline objects/s
   (`--gpus 1 --steps 5 --warmup 1`, without the CPU baseline and the prepass-off / low-precision legs) and the p50 of one KITTI-size
   detection (tools/gpu_detection_p50.py, 250 points + 200 free-space rays).  Acceptance: this tree's range overlaps the parent's own spread.
2. Cost with a mask ON: bench.py's cfg2x64 batch (`objects` objects of 2000 surface points + 500 free-space rays, 10 iterations) on ONE
   resident batch, settings interleaved, dsp_stats.ms_total: off; a mask of ones (= off, asserted bit for bit); the code frozen; the pose
   frozen.  No decoder or Gram work is skipped for frozen entries, so the masked runs are expected to cost what the plain run costs per
   launch; their trajectories differ, hence so may the number of samples decoded.
3. Tracking with rays: 16 synthetic KITTI-size detections, the ground-truth code, a perturbed pose (0.25 translation, up to 5 degrees
   yaw); pose error against the ground truth after N iterations for a pose-only batch (surface points only), a joint batch with the
   code frozen (points and rays), and the plain joint run.  Reported, not asserted.
4. --test-log: the figure lines tests/test_gpu_unknowns.py printed (`pytest -s`), copied in.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dsp_slam_amd import fixtures  # noqa: E402

LAUNCH_KEYS = ("n_mlp_fwd_launches", "n_mlp_jac_launches", "n_mlp_prepass_launches")


def _child(tree, args, seconds):
    """One measurement in a fresh process of `tree`; a failure ends the whole tool (nothing more is started on the GPU behind it)."""
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop("DSPGN_LIB", None)
    r = subprocess.run([sys.executable] + args, cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=seconds)
    if r.returncode != 0:
        sys.exit("%s in %s failed (%d):\n%s" % (" ".join(args), tree, r.returncode, r.stdout[-3000:]))
    return r.stdout


def ab(parent, rounds):
    out = {"bench": {"parent": [], "this": []}, "p50": {"parent": [], "this": []}, "min": {"parent": [], "this": []}}
    for _ in range(rounds):
        for name, tree in (("parent", parent), ("this", ROOT)):
            txt = _child(tree, ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1", "--no-cpu-baseline", "--no-prepass-off", "--no-lp"], 300)
            rec = json.loads([ln for ln in txt.splitlines() if ln.startswith("{")][-1])
            out["bench"][name].append(float(rec["value"]))
            txt = _child(tree, [os.path.join("tools", "gpu_detection_p50.py"), "30"], 120)
            line = [ln for ln in txt.splitlines() if "p50" in ln][-1]
            out["p50"][name].append(float(line.split("p50")[1].split("ms")[0]))
            out["min"][name].append(float(line.split("min")[1].split()[0]))
    return out


def ab_markdown(res, rounds):
    md = ["## Cost with the mask off: parent commit against this tree", "",
          "Fresh process per figure, order P N P N ..., %d rounds.  `bench.py --gpus 1 --steps 5 --warmup 1 --no-cpu-baseline --no-prepass-off --no-lp`" % rounds,
          "(cfg2x64, objects/s) and `tools/gpu_detection_p50.py 30` (one KITTI-size detection, 250 points + 200 free-space rays, ms).", "",
          "| figure | parent | this tree | parent spread | this tree's range | overlaps |", "|---|---|---|---|---|---|"]
    for key, label, fmt in (("bench", "headline, objects/s", "%.3f"), ("p50", "detection p50, ms", "%.4f"), ("min", "detection min, ms", "%.4f")):
        p, n = res[key]["parent"], res[key]["this"]
        spread = max(p) - min(p)
        overlap = min(n) <= max(p) + spread and max(n) >= min(p) - spread
        md.append("| %s | %s | %s | %s | %s .. %s | %s |" % (label, ", ".join(fmt % v for v in p), ", ".join(fmt % v for v in n), fmt % (max(p) - min(p)),
                                                       fmt % min(n), fmt % max(n), "yes" if overlap else "NO"))
    md += ["", "(overlaps: this tree's range meets the parent's range widened by the parent's own spread on either side.)", ""]
    return md


def _engine():
    from dsp_slam_amd import engine as E
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    sd = fixtures.load_decoder_npz(fixtures.fixture_path("cars"))
    layers = fold_weight_norm(sd, len(fixtures.SPECS["NetworkSpecs"]["dims"]) + 1)
    return E, E.Engine(layers, fixtures.SPECS["NetworkSpecs"]["latent_in"], fixtures.SPECS["CodeLength"], device=0)


def mask_cost(runs, n_objects):
    from dsp_slam_amd import synth
    E, eng = _engine()
    objs = synth.make_batch(n_objects, first_seed=1, n_surface=2000, n_background=500)
    b = eng.batch(E.gn_params(), [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs])
    settings = {"off": None, "ones": np.ones(71, np.uint8), "code frozen": ["pose"], "pose frozen": ["code"]}
    ms = {k: [] for k in settings}
    rows, launches, pts = {}, {}, {}
    for i in range(runs + 1):
        for name, live in settings.items():
            b.set_unknowns(live)
            b.run()
            st = b.stats()
            if i >= 1:
                ms[name].append(st["ms_total"])
            rows[name], launches[name] = b.results(), [st[k] for k in LAUNCH_KEYS]
            pts[name] = (st["n_fwd_points"] + st["n_prepass_points"], st["n_jac_points"] + st["n_render_rows"])
    b.close()
    eng.close()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(rows["off"], rows["ones"])), "a mask of ones changed a result bit"
    assert launches["off"] == launches["ones"], (launches["off"], launches["ones"])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    md = ["## Cost with a mask on: the headline batch", "",
          "%d objects of 2000 surface points + 500 free-space rays, 10 iterations, one resident batch, settings interleaved, %d timed runs each" % (n_objects, runs),
          "after one warm-up run each; `dsp_stats.ms_total` (HIP events around the run).  No work is skipped for frozen entries; a masked run",
          "follows another trajectory, so the samples its rays decode differ.", "",
          "| mask | median ms | min | max | against off | decoder launches (fwd, jac, prepass) | forward / prepass points | jacobian rows | good objects |", "|---|---|---|---|---|---|---|---|---|"]
    for name in settings:
        md.append("| %s | %.3f | %.3f | %.3f | %+.3f ms = %+.2f %% | %s | %.0f | %.0f | %d |" % (
            name, med[name], min(ms[name]), max(ms[name]), med[name] - med["off"], 100.0 * (med[name] - med["off"]) / med["off"], launches[name], pts[name][0],
            pts[name][1], int((rows[name][3] == 0).sum())))
    md += ["", "(`ones` returns the bits of `off` and launches the same kernels: asserted by the tool.)", ""]
    return md


def _pose_error(t, gt):
    t, gt = np.asarray(t, np.float64), np.asarray(gt, np.float64)
    sa, sb = np.cbrt(np.linalg.det(t[:3, :3])), np.cbrt(np.linalg.det(gt[:3, :3]))
    ang = np.degrees(np.arccos(np.clip((np.trace((t[:3, :3] / sa) @ (gt[:3, :3] / sb).T) - 1) / 2, -1, 1)))
    return float(np.linalg.norm(t[:3, 3] - gt[:3, 3])), float(ang), float(abs(np.log(sa / sb)))


def tracking(n_it):
    from dsp_slam_amd import synth
    E, eng = _engine()
    objs = synth.make_batch(16, first_seed=200, n_surface=250, n_background=200)
    codes = [np.concatenate([o["code_gt"], np.zeros(64 - o["code_gt"].shape[0], np.float32)]).astype(np.float32) for o in objs]
    prm = E.gn_params(num_iterations=n_it, pose_only_iterations=n_it)
    res = {"start": [o["t_cam_obj_init"] for o in objs]}
    se3, scales = [], []
    for o in objs:
        t = o["t_cam_obj_init"].astype(np.float64).copy()
        s = float(np.cbrt(np.linalg.det(t[:3, :3])))
        t[:3, :3] /= s
        se3.append(t.astype(np.float32))
        scales.append(s)
    poses = eng.estimate_pose_batch(prm, se3, scales, [o["pts"] for o in objs], codes)
    res["pose-only batch (points)"] = [np.vstack([np.hstack([s * p[:3, :3], p[:3, 3:4]]), [[0, 0, 0, 1]]]) for p, s in zip(poses, scales)]
    args = (prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs], codes)
    for name, unknowns in (("joint, code frozen (points + rays)", ["pose"]), ("joint, code and scale frozen", ["translation", "rotation"]), ("plain joint", None)):
        t, code, _, status = eng.reconstruct_batch(*args, unknowns=unknowns)
        res[name] = [t[i] if status[i] == 0 else np.full((4, 4), np.nan) for i in range(len(objs))]
    eng.close()
    md = ["## Tracking with rays", "",
          "16 synthetic KITTI-size detections (250 surface points, 200 free-space rays; seeds 200..215), the ground-truth code, a start pose 0.25 off in",
          "translation and up to 5 degrees off in yaw; error of the returned pose against the ground truth after %d iterations (median / max over the objects" % n_it,
          "that ended good).  Reported, not asserted.", "",
          "| configuration | translation | rotation, degrees | abs log scale | good |", "|---|---|---|---|---|"]
    for name, ts in res.items():
        e = np.array([_pose_error(t, o["t_cam_obj_gt"]) for t, o in zip(ts, objs)])
        ok = np.isfinite(e).all(1)
        md.append("| %s | %.4f / %.4f | %.3f / %.3f | %.4f / %.4f | %d |" % ((name,) + tuple(v for k in range(3) for v in (np.median(e[ok, k]), e[ok, k].max())) + (int(ok.sum()),)))
    md.append("")
    return md


def test_figures(path):
    keep = ("frozen ", "nothing live", "upright", "convergence rule", "step control", "prior block", "posterior,", "masked, guard", "worst figures", "pose-only, yaw")
    lines = [ln.lstrip(".").rstrip() for ln in open(path) if ln.lstrip(".").startswith(keep)]
    return ["## Figures the GPU tests printed (tests/test_gpu_unknowns.py, tests 2, 4, 5 and 7)", "", "```"] + lines + ["```", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--objects", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--test-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unknowns.md"))
    args = ap.parse_args()
    if args.test_log and not os.path.exists(args.test_log):
        sys.exit("no such file: %s" % args.test_log)
    md = ["# Mask of unknowns (dsp_batch_unknowns): measurements on an MI355X", "", "Written by `tools/measure_unknowns.py`.", ""]

    def add(section):          # the file is complete after every section: a later failure loses nothing measured
        md.extend(section)
        with open(args.out, "w") as f:
            f.write("\n".join(md) + "\n")
        print("\n".join(section), flush=True)
    if args.test_log:
        add(test_figures(args.test_log))
    if args.parent:
        add(ab_markdown(ab(os.path.abspath(args.parent), args.rounds), args.rounds))
    add(mask_cost(args.runs, args.objects))
    add(tracking(args.iterations))


if __name__ == "__main__":
    main()
