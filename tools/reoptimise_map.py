#!/usr/bin/env python3
"""Re-optimise every object of a saved DSP-SLAM map on the MI355X(s): the 1024-object job of BASELINE configs[3].

DSP-SLAM dumps its map at exit as MapObjects.txt -- id / 3x4 Sim(3) object->world pose / shape code per object
(src/System_util.cc:123-146; re-read by extract_map_objects.py:46-63).  The dump holds the RESULT of the per-detection optimisation, not
its inputs, so this tool takes the detections from a sidecar directory the caller fills while SLAM runs (one file per object, holding what
LocalMapping hands to Optimizer.reconstruct_object, src/LocalMapping_util.cc:179-180):

    <map_dir>/observations/<id>.npz :  pts (M,3) surface points, rays (R,3) ray directions (foreground rows first), depth (n_fg,)
                                       observed depths, all in the frame of the observing camera; t_world_cam (4,4) that camera's pose

An object seen from several key frames may have further files observations/<id>.<k>.npz (k = 1, 2, ...; same arrays, each with its own
t_world_cam): where any exist, the object is optimised over ALL its views -- one pose and one code, the first file's camera as the reference
camera (dsp_reconstruct_multiview).  A map without such files runs exactly as before.

Every object with an observation file is optimised jointly (shape code + Sim(3) pose) as ONE ragged batch per GPU, warm-started from the
saved code and pose: objects are block-sharded over the GPUs by estimated cost (dsp_slam_amd.distributed.shard_objects), each shard runs
as one dsp_batch on its own handle from its own host thread, and the result rows are gathered once.  Objects whose optimisation fails
(is_good False) or that have no observation keep their saved pose and code.  The map is written back in the reference's format.

    python tools/reoptimise_map.py --config configs/config_kitti.json --map_dir map/kitti/07 [--gpus N] [--out MapObjects.reopt.txt]

--tol POSE CODE (off without the flag) lets every object stop once its Gauss-Newton step is below the tolerances (dsp_batch_convergence).  The
iterations each object used are printed: how many a warm start saves depends on the map (profiles/early_stop.md).

--posterior FILE.npz writes, for every map object, the posterior record of the run (dsp_batch_posterior, "sum" weights: ids, status, info_pose,
cov_pose, var_code, loss, M, V, K; objects without an observation have status 1 = none), and prints which objects are poorly constrained.
The poses and codes written are bit for bit those of a run without the flag.  --posterior-level 2 (default 1) adds what a later run needs to take
the result back in as a prior: Lambda (71 x 71), g, t_obj_cam, code, and t_world_cam, the camera the record's pose is relative to.

--prior FILE.npz (a file written with --posterior-level 2) fuses those records into this run as a Gaussian prior on each object's pose and code
(dsp_batch_prior): objects are matched by id, a record that is not ok (or an object without one) gives no prior, and a record taken in another
camera is re-based (T0 <- T0 t_world_cam_old^-1 t_world_cam_new; the information lives in the object frame and does not change).  A record
already holds the k3 and k4 terms of its run: re-optimising with the same config counts them twice (include/dsp_gn.h).  The prior's chi2 at
each result is printed: a large value says the new data contradicts the old estimate.

--step-control L0 UP DOWN LMIN LMAX (off without the flag) switches Levenberg-Marquardt step control on (dsp_batch_step_control): a state is
kept only if it lowers the loss, a rejected step is solved again with more damping, and the loss written is the loss AT the returned state.
Conventional values: 0 10 0.1 1 inf.  The accepted / rejected counts are printed.  Not for maps with multi-view objects.

--reject PT_SDF RAY_RES (off without the flag) runs every shard twice on the SAME resident batch: once with the observation report, then --
with the surface points whose |sdf| exceeds PT_SDF and the rays whose |depth residual| exceeds RAY_RES at the first result given weight 0
(dsp_slam_amd.observations.reject, dsp_batch_observation_weights) -- once more from the same start; nothing is uploaded again but the two
weight arrays.  The second run's results are written; the rejected counts are printed.
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsp_slam_amd"))
sys.path.insert(0, ROOT)


def _read_observation(z):
    return dict(pts=np.ascontiguousarray(z["pts"], np.float32), rays=np.ascontiguousarray(z["rays"], np.float32),
                depth=np.ascontiguousarray(z["depth"], np.float32).reshape(-1), t_world_cam=np.asarray(z["t_world_cam"], np.float64))


def load_observations(map_dir, objs):
    """-> list parallel to objs: dict(pts, rays, depth, t_world_cam) or None."""
    out = []
    for o in objs:
        p = os.path.join(map_dir, "observations", "%d.npz" % o["id"])
        if not os.path.exists(p):
            out.append(None)
            continue
        z = np.load(p)
        ob = _read_observation(z)
        more, k = [], 1
        while os.path.exists(os.path.join(map_dir, "observations", "%d.%d.npz" % (o["id"], k))):      # further views of the same object
            more.append(_read_observation(np.load(os.path.join(map_dir, "observations", "%d.%d.npz" % (o["id"], k)))))
            k += 1
        if more:
            ob["more_views"] = more
        out.append(ob)
    return out


def object_views(ob):
    """The views of one observed object as dsp_reconstruct_multiview takes them: the first file's camera is the reference camera."""
    inv0 = np.linalg.inv(ob["t_world_cam"])
    views = [dict(t_ref_cam=np.eye(4, dtype=np.float32), pts=ob["pts"], rays=ob["rays"], depth=ob["depth"])]
    for v in ob.get("more_views", []):
        views.append(dict(t_ref_cam=(inv0 @ v["t_world_cam"]).astype(np.float32), pts=v["pts"], rays=v["rays"], depth=v["depth"]))
    return views


def iterations_histogram(iters):
    """'mean M over N objects; n: count, ...' of the iterations the observed objects used."""
    iters = np.asarray(iters, np.int64).reshape(-1)
    if iters.size == 0:
        return "no observed objects"
    vals, cnt = np.unique(iters, return_counts=True)
    return "mean %.2f over %d objects; %s" % (float(iters.mean()), iters.size, ", ".join("%d: %d" % (v, c) for v, c in zip(vals, cnt)))


def prior_arrays(prior, objs, obs, idx):
    """The --prior records matched to the observed objects idx: -> (t_obj_cam0 (n, 4, 4), code0 (n, 64), Lambda (n, 71, 71)); objects without
    an ok record get Lambda = 0 (no prior).  A record taken in another camera is re-based to the object's current reference camera."""
    n = len(idx)
    t0 = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    z0 = np.zeros((n, 64), np.float32)
    lam = np.zeros((n, 71, 71))
    row = {int(i): k for k, i in enumerate(np.asarray(prior["ids"]).reshape(-1))}
    for k, i in enumerate(idx):
        r = row.get(int(objs[i]["id"]))
        if r is None or int(prior["status"][r]) != 0:
            continue
        rebase = np.linalg.inv(np.asarray(prior["t_world_cam"][r], np.float64)) @ obs[i]["t_world_cam"]
        t0[k] = (np.asarray(prior["t_obj_cam"][r], np.float64) @ rebase).astype(np.float32)
        c = np.asarray(prior["code"][r], np.float32).reshape(-1)
        z0[k, :c.shape[0]] = c
        lam[k] = prior["Lambda"][r]
    return t0, z0, lam


def reoptimise(engines, prm, objs, obs, code_len, shards=None, compute=0, tol=None, posterior=None, posterior_level=1, prior=None,
               step_control=None, report=False, reject=None, unknowns=None):
    """objs / obs as read; engines: one dsp_slam_amd.engine.Engine per GPU.  -> (objects with updated pose / code, stats dict).
    shards: optional explicit (start, stop) blocks over the objects that have observations (default: cost-balanced over the engines).
    compute: 0 = fp32 (the parity path), 1 / 2 = the opt-in f16 / bf16 compute mode (include/dsp_gn.h: dsp_batch_set_compute).
    tol: None, or (pose_tol, code_tol[, min_iterations]): the per-object convergence rule; stats["iterations_used"] then holds the updates applied
    to every observed object (None without tol).
    posterior: None, "mean" or "sum": stats["posterior"] then holds Batch.posterior()'s level-1 arrays with one row per MAP object (status 1 =
    none for objects without an observation); posterior_level 2 adds Lambda, g, t_obj_cam, code and t_world_cam.
    prior: None, or the arrays of a level-2 posterior file (ids, status, t_obj_cam, code, Lambda, t_world_cam): prior_arrays;
    stats["prior_chi2"] then holds e^T Lambda e at each observed object's result (NaN: the object failed).
    step_control: None, or (lambda0, up, down, lambda_min, lambda_max) -- Batch.set_step_control; stats["step_decisions"] then holds
    (accepted, rejected) counted over all observed objects and iterations.
    report: True switches the observation report on (Batch.set_report); stats["report"] then maps "<object id>/<key>" to that object's rows
    (dsp_slam_amd.observations.object_rows: per-point sdf and alive bits, per-ray depth / hit / residual / counts, per-view sums), as
    numpy.savez takes them.
    reject: None, or (pt_sdf_max, ray_res_max): every shard runs with the report, turns it into 0 / 1 observation weights
    (observations.reject, Batch.set_observation_weights) and runs again on the same resident batch; everything returned is the second
    run's, and stats["rejected"] holds (points, rays) given weight 0, counted over all observed objects.
    unknowns: None, or the names of the LIVE groups of unknowns (dsp_slam_amd.engine.unknowns_mask: translation, rotation, yaw, scale, pose,
    code, all) -- Batch.set_unknowns; every other entry of every object keeps its value: ["pose"] tracks the poses with the map's codes
    held, ["code"] refits the shapes under the map's poses."""
    from dsp_slam_amd import distributed as D
    from dsp_slam_amd import observations as OBS
    if unknowns is not None:
        from dsp_slam_amd.engine import unknowns_mask
        unknowns_mask(list(unknowns))          # an unknown group name raises here, in front of any upload
    idx = [i for i, ob in enumerate(obs) if ob is not None]
    t_in, codes_in = [], []
    for i in idx:
        t_wc = obs[i]["t_world_cam"]
        t_in.append((np.linalg.inv(t_wc) @ np.asarray(objs[i]["pose"], np.float64)).astype(np.float32))     # object -> camera, the optimiser's frame
        codes_in.append(np.asarray(objs[i]["code"], np.float32)[:code_len])
    views = {i: object_views(obs[i]) for i in idx}
    if shards is None:
        shards = D.shard_objects([sum(D.object_cost(v["pts"].shape[0], v["rays"].shape[0], prm.num_depth_samples) for v in views[i]) for i in idx],
                                 len(engines))
    parts = [None] * len(shards)
    used = [None] * len(shards)
    post = [None] * len(shards)
    chi2 = [None] * len(shards)
    pri = None if prior is None else prior_arrays(prior, objs, obs, idx)
    multiview = any("more_views" in obs[i] for i in idx)
    if multiview and step_control is not None:
        raise ValueError("step control does not take multi-view objects")
    steps = [None] * len(shards)
    reports = [None] * len(shards)
    rejected = [None] * len(shards)
    if multiview and compute != 0:
        raise ValueError("the low-precision compute mode does not take multi-view objects")

    def work(r):
        a, b = shards[r]
        sel = idx[a:b]
        eng = engines[r % len(engines)]
        if (tol is not None or posterior is not None or pri is not None or step_control is not None or report or reject is not None or unknowns is not None) and b > a:      # the rule and the posterior live on resident batches: one per shard, created and destroyed here
            if multiview:
                bt = eng.multiview_batch(prm, t_in[a:b], [views[i] for i in sel], codes_in[a:b])
            else:
                bt = eng.batch(prm, t_in[a:b], [obs[i]["pts"] for i in sel], [obs[i]["rays"] for i in sel], [obs[i]["depth"] for i in sel], codes_in[a:b])
            try:
                if compute != 0:
                    bt.set_compute(compute)
                if tol is not None:
                    bt.set_convergence(*tol)
                if posterior is not None:
                    bt.set_posterior(posterior_level, posterior)
                if pri is not None:
                    bt.set_prior(pri[0][a:b], pri[1][a:b], pri[2][a:b])
                if step_control is not None:
                    bt.set_step_control(*step_control)
                if report or reject is not None:
                    bt.set_report(True)
                if unknowns is not None:
                    bt.set_unknowns(list(unknowns))
                bt.run()
                if reject is not None:      # report -> weights -> the same batch once more
                    pt_w, ray_w = OBS.reject(bt.report(), reject[0], reject[1])
                    rejected[r] = (int((pt_w == 0).sum()), int((ray_w == 0).sum()))
                    bt.set_observation_weights(pt_w, ray_w)
                    bt.set_report(bool(report))
                    bt.run()
                if report:
                    reports[r] = bt.report()
                if step_control is not None:
                    dec = bt.step_log()["decision"]
                    steps[r] = (int((dec == 1).sum()), int((dec == 2).sum()))
                parts[r] = D.pack_results(*bt.results())
                used[r] = bt.iterations_used()
                if posterior is not None:
                    post[r] = bt.posterior()
                if pri is not None:
                    chi2[r] = bt.prior_residual()["chi2"]
            finally:
                bt.close()
            return
        if multiview:      # one-view objects of such a map go through the same call: one view IS reconstruct_batch, bit for bit
            parts[r] = D.pack_results(*eng.reconstruct_multiview_batch(prm, t_in[a:b], [views[i] for i in sel], codes_in[a:b]))
            return
        res = eng.reconstruct_batch(prm, t_in[a:b], [obs[i]["pts"] for i in sel], [obs[i]["rays"] for i in sel], [obs[i]["depth"] for i in sel],
                                    codes_in[a:b], compute=compute)
        parts[r] = D.pack_results(*res)

    t0 = time.perf_counter()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(len(shards))]      # ctypes releases the GIL: one host thread per GPU
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    dt = time.perf_counter() - t0
    packed = np.concatenate([p for p in parts if p is not None and p.shape[0]], 0) if idx else np.zeros((0, D.RESULT_WIDTH), np.float32)
    t, codes, loss, status = D.unpack_results(packed)
    out = [dict(o) for o in objs]
    n_good = 0
    for k, i in enumerate(idx):
        if status[k] != 0:
            continue
        n_good += 1
        out[i]["pose"] = obs[i]["t_world_cam"] @ t[k].astype(np.float64)
        out[i]["code"] = codes[k, :len(objs[i]["code"])].astype(np.float32)
        out[i]["loss"] = float(loss[k])
    iters = None if tol is None else np.concatenate([u for u in used if u is not None] + [np.zeros(0, np.int32)])
    records = None
    if posterior is not None:
        n = len(objs)
        records = dict(ids=np.array([o["id"] for o in objs], np.int64), status=np.ones(n, np.int32), info_pose=np.zeros((n, 7, 7)), cov_pose=np.zeros((n, 7, 7)),
                       var_code=np.zeros((n, code_len)), loss=np.zeros(n, np.float32), M=np.zeros(n, np.int64), V=np.zeros(n, np.int64), K=np.zeros(n, np.int64))
        keys = ("status", "info_pose", "cov_pose", "var_code", "loss", "M", "V", "K")
        if posterior_level >= 2:
            records.update(Lambda=np.zeros((n, 71, 71)), g=np.zeros((n, 71)), t_obj_cam=np.zeros((n, 4, 4), np.float32), code=np.zeros((n, code_len), np.float32),
                           t_world_cam=np.tile(np.eye(4), (n, 1, 1)))
            keys += ("Lambda", "g", "t_obj_cam", "code")
            for i in idx:
                records["t_world_cam"][i] = obs[i]["t_world_cam"]
        k = 0
        for pr in post:
            if pr is None:
                continue
            m = pr["status"].shape[0]
            for key in keys:
                records[key][idx[k:k + m]] = pr[key]
            k += m
    prior_chi2 = None if pri is None else np.concatenate([c for c in chi2 if c is not None] + [np.zeros(0)])
    rows = None
    if report:
        from dsp_slam_amd.observations import object_rows
        rows, k = {}, 0
        for rp in reports:
            if rp is None:
                continue
            for j in range(len(rp["view_off"]) - 1):
                for key, val in object_rows(rp, j).items():
                    rows["%d/%s" % (objs[idx[k]]["id"], key)] = val
                k += 1
    step_decisions = None if step_control is None else tuple(int(sum(x[k] for x in steps if x is not None)) for k in (0, 1))
    n_rejected = None if reject is None else tuple(int(sum(x[k] for x in rejected if x is not None)) for k in (0, 1))
    return out, dict(rejected=n_rejected, step_decisions=step_decisions, prior_chi2=prior_chi2, n_objects=len(objs), n_observed=len(idx), n_good=n_good, seconds=dt, shards=[tuple(s) for s in shards], packed=packed,
                     iterations_used=iters, posterior=records, report=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--map_dir", required=True)
    ap.add_argument("--gpus", type=int, default=0, help="0 = every MI355X the library accepts")
    ap.add_argument("--out", default=None, help="default: <map_dir>/MapObjects.reopt.txt")
    ap.add_argument("--compute", choices=("f32", "f16", "bf16"), default="f32",
                    help="f32 = the parity path (default); f16 / bf16 = the opt-in low-precision compute mode: ~3.7 x the objects/s on large maps, accuracy in profiles/r06_lp_compute.md")
    ap.add_argument("--tol", type=float, nargs=2, metavar=("POSE", "CODE"), default=None,
                    help="stop each object once its Gauss-Newton step is below these tolerances (pose entries / code entries); off without the flag")
    ap.add_argument("--posterior", default=None, metavar="FILE.npz",
                    help="write every map object's posterior record (pose information / covariance, code variance, loss at the result) of this run")
    ap.add_argument("--posterior-level", type=int, choices=(1, 2), default=1,
                    help="2: the --posterior file also holds Lambda, g, the state and the camera of every record -- what --prior reads")
    ap.add_argument("--prior", default=None, metavar="FILE.npz",
                    help="fuse the records of an earlier run (written with --posterior FILE.npz --posterior-level 2) into this one as a Gaussian prior")
    ap.add_argument("--step-control", type=float, nargs=5, metavar=("L0", "UP", "DOWN", "LMIN", "LMAX"), default=None,
                    help="Levenberg-Marquardt step control: keep a state only if it lowers the loss (conventional: 0 10 0.1 1 inf); off without the flag")
    ap.add_argument("--report", default=None, metavar="FILE.npz",
                    help="write every observed object's observation report at its result, keyed '<object id>/<field>': per-point sdf and alive bits, per-ray "
                         "depth / hit / residual / counts, per-view sums (dsp_slam_amd.observations reads them)")
    ap.add_argument("--reject", type=float, nargs=2, metavar=("PT_SDF", "RAY_RES"), default=None,
                    help="run twice on the same resident batch: observations whose |sdf| / |depth residual| at the first result exceed these bounds get weight 0 in the second")
    ap.add_argument("--unknowns", default=None, metavar="GROUP[,GROUP...]",
                    help="the LIVE groups of unknowns out of translation, rotation, yaw, scale, pose, code, all; every other entry keeps the map's value "
                         "(pose: track the poses with the codes held; code: refit the shapes under the map's poses); every entry without the flag")
    args = ap.parse_args()
    from reconstruct.utils import get_configs
    from deep_sdf.workspace import config_decoder
    from dsp_slam_amd import _lib as L, engine as E
    from dsp_slam_amd.map_objects import read_map_objects, write_map_objects
    cfg = get_configs(args.config)
    objs = read_map_objects(os.path.join(args.map_dir, "MapObjects.txt"))
    obs = load_observations(args.map_dir, objs)
    n_dev = args.gpus or max(1, L.load().dsp_device_count())
    decoders = [config_decoder(cfg.DeepSDF_DIR).cuda(d) for d in range(n_dev)]        # one decoder (= one handle, one stream) per GPU
    prm = E.params_from_configs(cfg)
    out, st = reoptimise([d.engine for d in decoders], prm, objs, obs, cfg.optimizer.code_len, compute={"f32": 0, "f16": 1, "bf16": 2}[args.compute],
                         tol=None if args.tol is None else tuple(args.tol), posterior=None if args.posterior is None else "sum",
                         posterior_level=args.posterior_level, prior=None if args.prior is None else dict(np.load(args.prior)),
                         step_control=None if args.step_control is None else tuple(args.step_control),
                         report=args.report is not None, reject=None if args.reject is None else tuple(args.reject),
                         unknowns=None if args.unknowns is None else [g for g in args.unknowns.split(",") if g])
    dst = args.out or os.path.join(args.map_dir, "MapObjects.reopt.txt")
    write_map_objects(dst, out)
    print("re-optimised %d of %d objects (%d with observations) on %d GPU(s) in %.3f s = %.1f objects/s -> %s" % (
        st["n_good"], st["n_objects"], st["n_observed"], n_dev, st["seconds"], st["n_observed"] / max(st["seconds"], 1e-9), dst))
    if st["iterations_used"] is not None:
        print("iterations used: %s" % iterations_histogram(st["iterations_used"]))
    if st["rejected"] is not None:
        print("rejected after the first run: %d surface points, %d rays" % st["rejected"])
    if st["step_decisions"] is not None:
        print("step control: %d states accepted, %d rejected" % st["step_decisions"])
    if st["prior_chi2"] is not None:
        c = st["prior_chi2"]
        print("prior chi2 at the results: median %.3g, max %.3g over %d objects (%d failed)" % (
            float(np.nanmedian(c)) if np.isfinite(c).any() else float("nan"), float(np.nanmax(c)) if np.isfinite(c).any() else float("nan"), c.size,
            int(np.isnan(c).sum())))
    if st["report"] is not None:
        np.savez(args.report, **st["report"])
        print("observation report of %d objects -> %s" % (len({k.split("/")[0] for k in st["report"]}), args.report))
    if st["posterior"] is not None:
        rec = st["posterior"]
        np.savez(args.posterior, **rec)
        ok = rec["status"] == 0
        sd = np.sqrt(np.maximum(np.diagonal(rec["cov_pose"], axis1=1, axis2=2), 0.0))
        worst = np.argsort(-sd[:, 3:6].max(1) * ok)[:min(5, int(ok.sum()))]
        print("posterior records of %d objects (%d ok) -> %s; largest rotation standard deviations: %s" % (
            rec["status"].shape[0], int(ok.sum()), args.posterior, ", ".join("id %d: %.3g rad" % (rec["ids"][i], sd[i, 3:6].max()) for i in worst)))


if __name__ == "__main__":
    main()
