#!/usr/bin/env python3
"""What per-observation weights cost on the headline batch (needs an MI355X).

    python tools/measure_weights.py [--runs 9] [--objects 64]

Times bench.py's cfg2x64 batch (`objects` objects of 2000 surface points + 500 free-space rays, 10 iterations) on ONE resident batch in
three settings, interleaved, `runs` timed runs each after one warm-up run each; the figure is dsp_stats.ms_total (HIP events around the run
on the handle's stream):
    off    no weights: the launches of a library without the feature;
    ones   all weights 1: the weighted Gram instantiation and one weight-sum launch per iteration, on the same rows -- the feature's own cost
           (the results are those of `off`, bit for bit; asserted);
    drawn  weights uniform in [0.1, 4] with 10 % zeros: fewer rays are sampled, so the decoder's work shrinks with them.
The decoder launch counts of the three settings are printed beside the times (off and ones must agree).  profiles/observation_weights.md
holds the figures of one session.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dsp_slam_amd import fixtures  # noqa: E402

LAUNCH_KEYS = ("n_mlp_fwd_launches", "n_mlp_jac_launches", "n_mlp_prepass_launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--objects", type=int, default=64)
    args = ap.parse_args()
    from dsp_slam_amd import engine as E, synth
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm
    sd = fixtures.load_decoder_npz(fixtures.fixture_path("cars"))
    layers = fold_weight_norm(sd, len(fixtures.SPECS["NetworkSpecs"]["dims"]) + 1)
    eng = E.Engine(layers, fixtures.SPECS["NetworkSpecs"]["latent_in"], fixtures.SPECS["CodeLength"], device=0)
    objs = synth.make_batch(args.objects, first_seed=1, n_surface=2000, n_background=500)
    b = eng.batch(E.gn_params(), [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs])
    n_p, n_r = sum(o["pts"].shape[0] for o in objs), sum(o["rays"].shape[0] for o in objs)
    rng = np.random.default_rng(1)

    def drawn(n):
        w = rng.uniform(0.1, 4.0, n).astype(np.float32)
        w[rng.random(n) < 0.1] = 0.0
        return w
    settings = {"off": (None, None), "ones": (np.ones(n_p, np.float32), np.ones(n_r, np.float32)), "drawn": (drawn(n_p), drawn(n_r))}
    ms = {k: [] for k in settings}
    rows, launches = {}, {}
    for i in range(args.runs + 1):
        for name, (pw, rw) in settings.items():
            b.set_observation_weights(pw, rw)
            b.run()
            st = b.stats()
            if i >= 1:
                ms[name].append(st["ms_total"])
            rows[name], launches[name] = b.results(), [st[k] for k in LAUNCH_KEYS]
    b.close()
    eng.close()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(rows["off"], rows["ones"])), "unit weights changed a result bit"
    assert launches["off"] == launches["ones"], (launches["off"], launches["ones"])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for name in settings:
        print("headline batch, %d objects, %d timed runs: weights %-5s %.3f ms (min %.3f, max %.3f), %+.3f ms = %+.2f %% against off; decoder launches %s; good objects %d" % (
            args.objects, args.runs, name, med[name], min(ms[name]), max(ms[name]), med[name] - med["off"], 100.0 * (med[name] - med["off"]) / med["off"],
            launches[name], int((rows[name][3] == 0).sum())))


if __name__ == "__main__":
    main()
