#!/usr/bin/env python3
"""Measurements behind profiles/map_raycast.md (dsp_map_raycast), on one MI355X with the fixture decoders:

    python tools/measure_raycast.py render    [--repeats 7] [--out FILE.json]     # a. one 640 x 480 render of a 16-object map
    python tools/measure_raycast.py overshoot [--out FILE.json]                   # b. t_hit - t_true on rays toward surface points

a. times Engine.cast_rays against host_loop_march below: the same sphere tracing written as a user had to write it before dsp_map_raycast,
   one Engine.query_map per round on the world points of the live rays (a synchronisation, an upload and a host-built plan per round).
   The loop uses nothing dsp_map_raycast added.  Both are warmed up, then run alternately; medians and the spread (min .. max) are
   reported.  The decoder's share of the device time (dsp_debug_query_timing events) comes from runs of their own, and the rows per round
   from the calls' stats.
b. projects 100 points onto each fixture decoder's zero set (Engine.surface_points), casts toward each from 1.5 s out along its normal
   and reports the distribution of t_hit - t_true, t_true the distance to the projected point, at the default eps / relax and at relax 0.5.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32 = np.float32


def engine(name):
    from oracle import dsp_oracle as O
    from dsp_slam_amd import fixtures, engine as E
    dec = O.fold_decoder(fixtures.load_decoder_npz(fixtures.fixture_path(name)), fixtures.fixture_specs(name))
    return E.Engine(dec.layers, dec.latent_in, dec.code_len, device=0)


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.sqrt((q * q).sum(1))[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def scene16(rng):
    """16 objects on a 4 x 4 grid, 2 apart, scales 0.9 .. 1.2 (neighbouring spheres overlap), random rotations; a camera above one corner
    looking at the middle."""
    n = 16
    t = np.zeros((n, 4, 4))
    t[:, :3, :3] = rotations(rng, n) * rng.uniform(0.9, 1.2, n)[:, None, None]
    t[:, :3, 3] = [[2.0 * (k % 4), 2.0 * (k // 4), 0.0] for k in range(n)]
    t[:, 3, 3] = 1
    codes = list(rng.uniform(-0.3, 0.3, (n, 64)).astype(F32))
    eye, at = np.array([-1.0, -1.0, 1.8]), np.array([3.0, 3.0, 0.0])
    z = (at - eye) / np.linalg.norm(at - eye)
    x = np.cross(z, [0, 0, 1.0])
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return t.astype(F32), codes, T


def sphere_entries(t, org, u):
    """float64: per (object, ray) the parameters where the ray enters and leaves the object's sphere (nan where it misses)."""
    t = t.astype(np.float64)
    c = t[:, :3, 3]
    r = np.cbrt(np.linalg.det(t[:, :3, :3]))
    oc = org[None] - c[:, None]
    b = (oc * u[None]).sum(2)
    disc = b * b - ((oc * oc).sum(2) - (r * r)[:, None])
    with np.errstate(invalid="ignore"):
        q = np.sqrt(disc)
    return -b - q, -b + q


def host_loop_march(eng, t, codes, org, dirs, eps, relax, max_steps, timed=False):
    """Sphere tracing of the map by a host loop over Engine.query_map: every round queries the live rays' world points; dist <= eps is a
    hit; inside a sphere the ray advances by relax * dist; outside every sphere it jumps to its next sphere entry (or ends)."""
    org64 = org.astype(np.float64)
    u = dirs.astype(np.float64)
    u /= np.sqrt((u * u).sum(1))[:, None]
    t_in, t_out = sphere_entries(t, org64, u)
    t_in = np.maximum(t_in, 0.0) + 1e-4                 # a hair inside, so that the query finds the sample in the sphere
    t_in = np.where(np.isfinite(t_in) & (t_out > t_in), t_in, np.inf)                     # entries still ahead of the origin
    n = org.shape[0]
    tcur = t_in.min(0)
    obj, t_hit, dist = np.full(n, -1, np.int32), np.full(n, np.inf, F32), np.full(n, np.inf, F32)
    live = np.flatnonzero(np.isfinite(tcur))
    rows, rounds, dec_ms, dev_ms = [], 0, 0.0, 0.0
    ms2 = np.zeros(2)
    from dsp_slam_amd import _lib as L
    for _ in range(max_steps):
        if live.size == 0:
            break
        p = (org64[live] + tcur[live, None] * u[live]).astype(F32)
        r = eng.query_map(t, codes, p)
        if timed:                                       # the caller has switched the handle's event brackets on
            L.load().dsp_debug_query_timing(eng._h, 1, L.ptr(ms2, L.c_f64p))
            dec_ms += ms2[0]
            dev_ms += ms2[1]
        rows.append(eng.query_stats()["rows"])
        rounds += 1
        hit = (r["obj"] >= 0) & (r["dist"] <= F32(eps))
        obj[live[hit]], t_hit[live[hit]], dist[live[hit]] = r["obj"][hit], tcur[live[hit]].astype(F32), r["dist"][hit]
        inside = (r["obj"] >= 0) & ~hit
        tcur[live[inside]] += relax * r["dist"][inside].astype(np.float64)
        out = np.flatnonzero(r["obj"] < 0)              # outside every sphere (or past the last sample's): the next entry ahead
        ahead = np.where(t_in[:, live[out]] > tcur[live[out]][None, :], t_in[:, live[out]], np.inf).min(0)
        tcur[live[out]] = ahead
        live = live[~hit & np.isfinite(tcur[live])]
    return {"obj": obj, "t": t_hit, "dist": dist}, {"rows": rows, "rounds": rounds, "decoder_ms": dec_ms, "device_ms": dev_ms}


def measure_render(args):
    from dsp_slam_amd import _lib as L, map_objects as M
    eng = engine("cars")
    t, codes, T = scene16(np.random.default_rng(90))
    W, H = 640, 480
    org, dirs, _ = M.pixel_rays((320.0, 320.0, 319.5, 239.5), T, W, H)
    prm = eng.raycast_params()
    eps, relax, steps = float(prm.eps), float(prm.relax), int(prm.max_steps)
    new_s, loop_s = [], []
    for k in range(2 + args.repeats):                   # two warm-up runs of both, then alternating; no event brackets in the timed runs
        t0 = time.perf_counter()
        res = eng.cast_rays(t, codes, org, dirs)
        dt_new = time.perf_counter() - t0
        st = eng.raycast_stats()
        t0 = time.perf_counter()
        ref, loop_info = host_loop_march(eng, t, codes, org, dirs, eps, relax, steps)
        dt_loop = time.perf_counter() - t0
        if k >= 2:
            new_s.append(dt_new); loop_s.append(dt_loop)
    # the device's split, in runs of their own: events around every call and every decoder launch inside it
    ms2, new_ms = np.zeros(2), []
    L.load().dsp_debug_query_timing(eng._h, 1, None)
    for k in range(3):
        eng.cast_rays(t, codes, org, dirs)
        L.load().dsp_debug_query_timing(eng._h, 1, L.ptr(ms2, L.c_f64p))
        new_ms.append(ms2.copy())
        _, loop_info = host_loop_march(eng, t, codes, org, dirs, eps, relax, steps, timed=True)
    L.load().dsp_debug_query_timing(eng._h, 0, None)
    new_ms = np.median(np.array(new_ms), 0)
    both = (res["obj"] >= 0) & (ref["obj"] >= 0)
    out = {"what": "render 640x480, 16 objects, cars decoder", "eps": eps, "relax": relax, "max_steps": steps, "repeats": args.repeats,
           "cast_rays_s": {"median": float(np.median(new_s)), "min": float(min(new_s)), "max": float(max(new_s))},
           "host_loop_s": {"median": float(np.median(loop_s)), "min": float(min(loop_s)), "max": float(max(loop_s))},
           "ratio_loop_over_cast": float(np.median(loop_s) / np.median(new_s)),
           "cast_rays_device_ms": {"decoder": float(new_ms[0]), "whole_call": float(new_ms[1])},
           "host_loop_device_ms": {"decoder": loop_info["decoder_ms"], "whole_calls": loop_info["device_ms"]},
           "cast_rays_stats": st, "cast_rays_rows_per_round": st["rows"] / max(1, st["rounds"]),
           "host_loop_rounds": loop_info["rounds"], "host_loop_rows": loop_info["rows"],
           "pixels_hit": {"cast_rays": int((res["obj"] >= 0).sum()), "host_loop": int((ref["obj"] >= 0).sum()), "both": int(both.sum()),
                          "same_object": int((res["obj"][both] == ref["obj"][both]).sum()),
                          "median_abs_dt": float(np.median(np.abs(res["t"][both].astype(np.float64) - ref["t"][both]))) if both.any() else None},
           "undecided": int((res["status"] == 2).sum())}
    eng.close()
    return out


def measure_overshoot(args):
    out = {"what": "t_hit - t_true, 100 rays toward projected surface points from 1.5 s out along the normal", "decoders": {}}
    for name in ("cars", "chairs32", "complex"):
        eng = engine(name)
        rng = np.random.default_rng(76)
        t0 = np.eye(4)
        t0[:3, :3] = rotations(np.random.default_rng(41), 3)[0] * 0.8
        scale = 0.8
        code = np.random.default_rng(42).uniform(-0.3, 0.3, (3, 64)).astype(F32)[0][:eng.code_len]
        start = rng.normal(size=(100, 3))
        start = 0.35 * start / np.sqrt((start * start).sum(1))[:, None]
        sp = eng.surface_points([code], [start.astype(F32)], steps=8)[0]
        p_w = sp["vertices"].astype(np.float64) @ t0[:3, :3].T
        n_w = sp["normals"].astype(np.float64) @ (t0[:3, :3] / scale).T
        org = (p_w + 1.5 * scale * n_w).astype(F32)
        dirs = (p_w - org.astype(np.float64)).astype(F32)
        t_true = np.sqrt(((p_w - org.astype(np.float64)) ** 2).sum(1))
        rec = {"max_abs_sdf_at_projected_points": float(np.abs(sp["sdf"]).max())}
        for relax in (1.0, 0.5):
            r = eng.cast_rays(t0[None].astype(F32), [code], org, dirs, relax=relax)
            hit = r["status"] == 1
            d = r["t"][hit].astype(np.float64) - t_true[hit]
            st = eng.raycast_stats()
            rec["relax_%g" % relax] = {"hits": int(hit.sum()), "undecided": int((r["status"] == 2).sum()), "rows": st["rows"], "rounds": st["rounds"],
                                       "min": float(d.min()), "p10": float(np.percentile(d, 10)), "median": float(np.median(d)),
                                       "p90": float(np.percentile(d, 90)), "max": float(d.max()), "scale": scale}
        out["decoders"][name] = rec
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["render", "overshoot"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = measure_render(args) if args.what == "render" else measure_overshoot(args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
