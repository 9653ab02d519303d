#!/usr/bin/env python3
"""What Levenberg-Marquardt step control (dsp_batch_step_control) does to the returned loss and what it costs: the tables of
profiles/step_control.md.

64 cfg2-size objects built as bench.py builds them (2000 surface points + 500 background rays, seeds 1..64), cold, and one detection-sized
object (250 + 200, seed 4242).  Rows: the plain 10 iterations; step control (0, 10, 0.1, 1, inf) at 10, 14 and 20 iterations and at 20 with
dsp_batch_convergence(1e-3, 1e-3, 1); and, at 14 iterations, a small sweep of `up` over {2, 10} and `lambda_min` over {0.1, 1, 10}.
Per row: objects/s (wall clock around run + results, median of --runs), mean iterations used, accepted / rejected decisions, median and
worst returned loss beside the plain run's, and the share of objects whose returned loss is lower than the plain run's.

A second table gives the per-iteration time with the feature on against the same batch with it off (same iteration count), for the
six-object batch of tests/test_gpu_step_control.py, the 64-object batch and the detection.

    python tools/measure_step_control.py [--runs 5] [--objects 64]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INF = float("inf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--objects", type=int, default=64)
    args = ap.parse_args()
    from dsp_slam_amd import fixtures, synth, engine as E
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    sd = fixtures.load_decoder_npz(fixtures.fixture_path("cars"))
    layers = fold_weight_norm(sd, len(fixtures.SPECS["NetworkSpecs"]["dims"]) + 1)
    eng = E.Engine(layers, fixtures.SPECS["NetworkSpecs"]["latent_in"], fixtures.SPECS["CodeLength"], device=0)
    prm = E.gn_params()

    def batch(objs):
        return eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs],
                         [np.zeros(64, np.float32) for _ in objs])

    def timed(b):
        b.run()
        dt = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            b.run()
            res = b.results()
            dt.append(time.perf_counter() - t0)
        return statistics.median(dt), res

    def measure(name, objs):
        b = batch(objs)
        rows = [("plain", 10, None, None)]
        rows += [("step control", n, (0.0, 10.0, 0.1, 1.0, INF), None) for n in (10, 14, 20)]
        rows += [("step control + convergence(1e-3, 1e-3, 1)", 20, (0.0, 10.0, 0.1, 1.0, INF), (1e-3, 1e-3, 1))]
        rows += [("step control, up %g lambda_min %g" % (up, lmin), 14, (0.0, up, 0.1, lmin, INF), None) for up in (2.0, 10.0) for lmin in (0.1, 1.0, 10.0)]
        ref = None
        for label, n_it, sc, conv in rows:
            b.set_iterations(n_it)
            b.set_step_control(*(sc or (0.0,) * 5))
            b.set_convergence(*(conv or (0.0, 0.0, 1)))
            sec, res = timed(b)
            used = b.iterations_used()
            if ref is None:
                ref = res
            acc = rej = 0
            if sc is not None:
                dec = b.step_log()["decision"]
                acc, rej = int((dec == 1).sum()), int((dec == 2).sum())
            good = (ref[3] == 0) & (res[3] == 0)
            loss, loss0 = res[2][good].astype(np.float64), ref[2][good].astype(np.float64)
            print("| %s | %s | %d | %.1f | %.3f | %.2f | %d | %d | %.4f (%.4f) | %.4f (%.4f) | %.0f %% | %d |" % (
                name, label, n_it, len(objs) / sec, sec * 1e3, float(used.mean()), acc, rej, float(np.median(loss)), float(np.median(loss0)),
                float(loss.max()), float(loss0.max()), 100.0 * float((loss < loss0).mean()), int((res[3] == 0).sum())), flush=True)
        b.close()

    print("| batch | rule | iterations | objects/s | ms per run | mean iterations used | accepted | rejected | median returned loss (plain) | worst returned loss (plain) | "
          "objects with a lower loss than plain | good |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    cold = synth.make_batch(args.objects, first_seed=1, n_surface=2000, n_background=500)
    det = [synth.make_object(4242, n_surface=250, n_background=200)]
    measure("%d cfg2 objects, cold" % args.objects, cold)
    measure("1 detection, cold", det)

    print()
    print("| batch | iterations | ms per iteration, off | ms per iteration, on | difference |")
    print("|---|---|---|---|---|")
    six = [synth.make_object(300, n_surface=160, n_background=40), synth.make_object(301, n_surface=160, n_background=40),
           synth.make_object(302, n_surface=160, n_background=40, t_noise=0.6, yaw_noise_deg=15.0)]
    six = six + six
    for name, objs in (("6 objects (160 + 200)", six), ("%d cfg2 objects" % args.objects, cold), ("1 detection", det)):
        b = batch(objs)
        b.set_iterations(10)
        ms = {}
        for on in (False, True, False, True):          # interleaved: off, on, off, on; the better of the two medians each
            b.set_step_control(*((0.0, 10.0, 0.1, 1.0, INF) if on else (0.0,) * 5))
            sec, _ = timed(b)
            ms[on] = min(ms.get(on, 1e9), sec * 1e3 / 10)
        print("| %s | 10 | %.4f | %.4f | %+.1f %% |" % (name, ms[False], ms[True], 100.0 * (ms[True] / ms[False] - 1.0)), flush=True)
        b.close()
    eng.close()


if __name__ == "__main__":
    main()
