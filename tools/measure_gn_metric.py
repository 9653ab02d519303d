#!/usr/bin/env python3
"""The fp64 Gauss-Newton systems at the reference's recorded states, and how far the fp32 oracle and the reference sit from them.

    python tools/measure_gn_metric.py --measure out.json [--recon-only]   # scaled errors (tests/gn_metric.py) at every recorded state -> json

For every recorded state -- camera->object matrix, code and depth samples of iteration e of a golden_recon_*.npz, or of a traced object of
golden_bench_cfg2x64.npz -- the fp32 oracle linearises on the recorded depth samples (this decides the sample sets, and its V and K must be
the reference's), then oracle.dsp_oracle.linearise_fp64 evaluates the same system in float64 on those sets.

    python tools/measure_gn_metric.py --multiview [golden] [cases] [faults]  # the multi-view tables of profiles/multiview_metric.md

--multiview prints, against the pooled fp64 system (oracle.dsp_oracle.linearise_fp64_multiview) on the composed fp32 oracle's sets: the
composed oracle, its sdf-jitter twin and the reference's recorded system at every iteration of golden_multiview_cars3.npz; every iteration
of the composed oracle's own run on each case of tests/multiview_metric.py; and the six member-view faults with the max-norm verdict.

--measure writes, per state, the scaled errors of the fp32 oracle's and of the reference's recorded system against fp64, without the
sdf-jitter allowance (the numbers tests/gn_metric.py derives its TAU from).  CPU only; reads nothing outside the repository.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import dsp_oracle as O  # noqa: E402
from dsp_slam_amd import fixtures, synth  # noqa: E402
import forensics as F  # noqa: E402
import gn_metric as M  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
RECON = ["small", "cfg1", "cfg2", "cfg5", "redwood", "freiburg", "chairs32", "complex"]
BENCH = "golden_bench_cfg2x64.npz"


def decoder_for(cfg):
    name = os.path.basename(cfg.get("DeepSDF_DIR", "cars"))
    fix = "complex" if name.startswith("complex") else ("chairs32" if cfg["optimizer"]["code_len"] == 32 else "cars")
    return O.fold_decoder(fixtures.load_decoder_npz(fixtures.fixture_path(fix)), fixtures.fixture_specs(fix))


def recorded_states(recon_only=False):
    """-> [(case, iteration, decoder, prm, inputs (pts, rays, depth), state (t_obj_cam, code, depths), reference system (H, b, dx))]"""
    decs = {}
    for r in RECON:
        g = np.load(os.path.join(GOLD, "golden_recon_%s.npz" % r))
        cfg = json.loads(str(g["cfg_json"]))
        key = json.dumps(cfg.get("DeepSDF_DIR")) + str(cfg["optimizer"]["code_len"])
        dec = decs.setdefault(key, decoder_for(cfg))
        prm = O.GNParams.from_configs(cfg)
        for e in range(g["it_H"].shape[0]):
            yield (r, e, dec, prm, (g["in_pts"], g["in_rays"], g["in_depth"]), (g["it_t_obj_cam"][e], g["it_code"][e], g["it_depths"][e]),
                   dict(H=g["it_H"][e], b=g["it_b"][e], dx=g["it_dx"][e]), (int(g["it_V"][e]), int(g["it_K"][e])))
    if not recon_only:
        yield from bench_states()


def bench_states():
    g = np.load(os.path.join(GOLD, BENCH))
    cfg = json.loads(str(g["cfg_json"]))
    prm = O.GNParams.from_configs(cfg)
    dec = decoder_for(cfg)
    objs = synth.make_batch(int(g["all_it_V"].shape[0]), first_seed=int(g["first_seed"]), n_surface=int(g["n_surface"]),
                            n_background=int(g["n_background"]))
    for i in [int(i) for i in g["full_objects"]]:
        o, p = objs[i], "tr%d_" % i
        for e in range(g[p + "it_H"].shape[0]):
            yield ("bench%d" % i, e, dec, prm, (o["pts"], o["rays"], o["depth"]), (g[p + "it_t_obj_cam"][e], g[p + "it_code"][e], g[p + "it_depths"][e]),
                   dict(H=g[p + "it_H"][e], b=g[p + "it_b"][e], dx=g[p + "it_dx"][e]), (int(g[p + "it_V"][e]), int(g[p + "it_K"][e])))


def linearise(dec, prm, inputs, state):
    """-> (fp32 oracle trace, fp64 linearisation on its sets)."""
    it = F.oracle_linearisation(dec, prm, *inputs, *state)
    return it, O.linearise_fp64(dec, prm, *inputs, *state, it["sets"])


def _worst(rec):
    return "H %.1e b %.1e dx %.1e solve %.1e" % (max(rec["H"].values()), max(rec["b_pose"], rec["b_code"]), rec["dx"], rec["solve"])


def multiview(parts):
    import multiview_metric as X
    import multiview_oracle as MV
    decs = {"cars": decoder_for({"optimizer": {"code_len": 64}}), "chairs32": decoder_for({"optimizer": {"code_len": 32}})}
    if "golden" in parts:
        g = np.load(os.path.join(GOLD, "golden_multiview_cars3.npz"))
        prm = O.GNParams.from_configs(json.loads(str(g["cfg_json"])))
        views = MV.golden_views(g)
        print("golden_multiview_cars3.npz: scaled errors against the pooled fp64 (no jitter allowance)")
        for e in range(g["it_H"].shape[0]):
            t0 = time.time()
            it, itj, lin = X.linearise_at(decs["cars"], prm, views, g["it_t_obj_cam"][e], g["it_code"][e], g["it_depths"][e])
            ref = dict(H=g["it_H"][e], b=g["it_b"][e], dx=g["it_dx"][e])
            print("  it %d V %s K %s n_flip %s (%.1f s)" % (e, lin["V_views"], lin["K_views"], lin["n_flip"], time.time() - t0))
            for who, s in (("oracle", it), ("jitter twin", itj), ("reference", ref)):
                print("    %-12s %s" % (who, _worst(M.scaled_errors(s, lin, prm.k4))), flush=True)
    if "cases" in parts:
        for name, make in X.CASES.items():
            case = make()
            oprm = X.oracle_params(case)
            for i, obj in enumerate(case["objects"]):
                t0 = time.time()
                run = X.own_run(decs[case["decoder"]], oprm, obj, case["n_it"])
                print("%s object %d (%d views): %d iterations of the composed oracle's own run (%.1f s)" % (name, i, len(obj["views"]), len(run), time.time() - t0))
                for e, (it, itj, lin) in enumerate(run):
                    print("  it %d (V, K) %s M %d K %d jitter twin's sets %s n_flip %s: %s" % (
                        e, X.view_vk(it), it["M"], it["K"], "same" if X.same_sets(it, itj) else "DIFFER", lin["n_flip"],
                        _worst(M.scaled_errors(it, lin, oprm.k4))), flush=True)
    if "faults" in parts:
        for label, oprm, views, it, lin, prev_code in X.fault_states(decs["cars"]):
            base = M.scaled_errors(it, lin, oprm.k4)
            print("%s: unperturbed worst %.1e (%s)" % (label, base["worst"], "accepted" if M.within_tau(base) else "REJECTED"))
            for what, sys_ in X.faults(decs["cars"], oprm, views, it, prev_code).items():
                rec = M.scaled_errors(sys_, lin, oprm.k4)
                print("  %-62s worst %.1e solve %.1e %-8s max-norm check: %s" % (
                    what, rec["worst"], rec["solve"], "accepted" if M.within_tau(rec) else "rejected", "passes" if X.max_norm_passes(sys_, it, oprm.k4) else "fails"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multiview", nargs="*", choices=["golden", "cases", "faults"], help="print the multi-view tables (default: all three)")
    ap.add_argument("--measure", help="write the per-state scaled errors of the oracle and the reference to this json")
    ap.add_argument("--recon-only", action="store_true", help="the golden_recon_* states only (not the 160 bench iterations)")
    ap.add_argument("--bench-only", action="store_true", help="the 160 bench iterations only")
    a = ap.parse_args()
    if a.multiview is not None:
        multiview(a.multiview or ["golden", "cases", "faults"])
    if a.measure:
        rows = []
        for case, e, dec, prm, inputs, state, ref, vk in (bench_states() if a.bench_only else recorded_states(a.recon_only)):
            t0 = time.time()
            it, lin = linearise(dec, prm, inputs, state)
            assert (it["V"], it["K"]) == vk, (case, e, "the oracle's sets differ from the reference's")
            row = dict(case=case, it=e, K=it["K"], n_flip=lin["n_flip"])
            for who, s in (("oracle", it), ("ref", ref)):
                row[who] = M.flat(M.scaled_errors(s, lin, prm.k4))
            row["seconds"] = time.time() - t0
            rows.append(row)
            print(case, e, " ".join("%s %.2e" % (k, max(v for q, v in row[k].items() if q != "solve")) for k in ("oracle", "ref")),
                  "solve %.1e / %.1e (%.1f s)" % (row["oracle"]["solve"], row["ref"]["solve"], row["seconds"]), flush=True)
            with open(a.measure, "w") as f:
                json.dump(rows, f, indent=0)


if __name__ == "__main__":
    main()
