#!/usr/bin/env python3
"""Benchmark of the DeepSDF shape/pose Gauss-Newton hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 5 --warmup 1 [--config cfg2x64|cfg4|cfg5] [--prepass auto|off|f16|bf16] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W [--full]

One "step" = one pass of the hot path (Optimizer.reconstruct_object, every GN iteration) over one batch of synthetic
objects per GPU, inputs already resident in HBM (dsp_batch_create uploads them before the timed region), followed by one
RCCL gather of the per-object results (pose 16 + code 64 + loss + status floats) to rank 0.  Objects are independent, so
ranks shard them with no other collective: weak scaling, value = objects of all ranks / max-over-ranks time.

Workloads (BASELINE.json configs):
  cfg2x64 (default; the configuration the metric is quoted on): 64 cfg2 objects per GPU -- 2000 surface points + 500
          background rays x 50 depth samples, 64-D code, 10 iterations, KITTI hyper-parameters;
  cfg4    BASELINE configs[3] as written: a FIXED job of 1024 cfg2 objects (--total-objects) block-sharded over the N GPUs by
          distributed.shard_objects (--partition static | measured): "scaling": "strong"; --objects-per-gpu makes it a weak-scaling run;
  cfg5    4000-point objects, Redwood hyper-parameters (5 iterations), a mixed batch on two resident decoders (cars, 64-D codes +
          chairs32, 32-D codes and its own weights), 32 + 32 objects per GPU.

--dump-outputs DIR writes what the last timed step of the headline run returned -- the result rows of every object of every rank, in
object order, as Batch.results() hands them to a caller -- to DIR/t_cam_obj.npy (N, 4, 4), DIR/code.npy (N, 64; a 32-D code fills the first
32 columns), DIR/loss.npy (N,) and DIR/status.npy (N,; 0 = good), all float32.  The inputs are seeded, so two builds run with the same
arguments can be compared output for output.

A plain run does only what the headline figure needs: set up, warm up, time the steps, write --dump-outputs, print the JSON line.  Besides
`value`, `ms_per_step` and `dtype` that line carries what the headline's own steps measured (HIP events around every decoder launch):
  roofline      fp32-MFMA roofline of the dominant fp32 kernel (forward decoder with relu-mask export, mlp_kernel<1>):
                algorithmic FLOPs = points the launches actually decode x 3 671 040 FLOP / HIP-event time
                of those launches;
  prepass       the low-precision classification kernel in front of it (mlp_lp_kernel, f16 MFMA), priced SEPARATELY
                against the dense 16-bit MFMA peak -- never mixed into the fp32 fraction;
  by_rank       every rank's own fractions, guard counters, sum of V and K, per-kernel ms.

--full adds, after the headline leg and in this order, the legs that take runs of their own (--no-prepass-off, --no-lp, --no-cpu-baseline
and --latency-runs trim them; a plain run ignores those four):
  prepass_off   the same batch timed in the same run, over the same number of steps, with the prepass OFF (every in-sphere sample through
                the fp32 kernel, as the reference evaluates it): objects/s (= the top-level `value_fp32_only`), ms_per_step and the fp32
                kernel's roofline fraction of THAT run; `dtype` says what the headline computed in ("f32 + f16 classifier");
  lp_compute    the same batch in the opt-in low-precision compute mode (16-bit MFMA operands, fp32 accumulation) over as many steps: its
                objects/s (= the top-level `value_lp`), rooflines, and how far its results sit from the fp32 path's (cfg2x64 only);
  prepass.sustained_clock_mhz
                the shader clock granted under a bare prepass decode (also by_rank[].prepass_clock_mhz; null in a plain run);
  latency_ms_p50, latency_kitti_size_ms_p50, latency_one_shot_ms_p50, pose_only
                one-object latencies and the pose-only batch (N=1, cfg2x64 only);
  cpu_baseline  the reference itself (kind "reference") when DSP_REFERENCE_ROOT points at a DSP-SLAM checkout, else
                oracle/torch_baseline.py (kind "port", `port` = "torch-restatement": the reference's own torch op sequence written out, bit-identical
                results; `calibrated_vs_reference` = its time / the unmodified reference's, measured in the build container,
                profiles/cpu_baseline_calibration.json), timed on this box's host cores on one warm-up + THREE cfg2 objects (rank 0, N=1 only;
                objects/s = 1 / mean, p50 alongside: BASELINE.md section 2) -- a reported baseline, not a target.

roofline.rocprof_check lists per LEG of this process (headline warm-up / timed, then the legs --full adds) the launch counts and HIP-event
averages of the decoder kernels.  Every leg opens with one launch of a marker kernel (k_debug_lie), so tools/rocpd_legs.py can split a
rocprofv3 kernel trace of the same command at the marker dispatches and compare each population of a kernel with its own figure
(profiles/rNN_kernel_stats.md).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F_FWD = 3671040.0          # FLOP / point, decoder forward                
F_JAC = 7342080.0          # FLOP / point, forward + input-gradient
PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: 256 CU x 256 FLOP/clk x 2.4 GHz
PEAK_16BIT_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 / f16 MFMA (no sparsity)
REDWOOD = dict(k1=10.0, k2=100.0, k3=2.5, k4=0.0, b1=0.2, b2=0.02, lr=1.0, s_damp=100.0, num_iterations=5)   # config_redwood_01053.json
PREPASS = {"auto": -1, "off": 0, "f16": 1, "bf16": 2}


def reference_cpu_baseline(obj, threads):
    """Time the UNMODIFIED reference (reconstruct/optimizer.py, torch CPU) on one object on the host cores.  Only attempted when
    DSP_REFERENCE_ROOT names a DSP-SLAM checkout (oracle/ref_shim.py imports it in place); returns None otherwise."""
    try:
        import tempfile
        import torch
        from oracle import ref_shim         # stubs addict / plyfile / skimage, neutralises the reference's .cuda() calls
        from dsp_slam_amd import fixtures
        if not ref_shim.reference_available():
            return None
        ref_shim.install(force_cpu=True)
        from reconstruct.utils import get_configs, get_decoder
        from reconstruct.optimizer import Optimizer
        d = tempfile.mkdtemp(prefix="dsp_ref_")
        cars_dir = fixtures.materialize_decoder_dir("cars", os.path.join(d, "cars_64"))
        cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
        cfg["DeepSDF_DIR"] = cars_dir
        with open(os.path.join(d, "cfg.json"), "w") as f:
            json.dump(cfg, f)
        cfg = get_configs(os.path.join(d, "cfg.json"))
        torch.set_num_threads(threads)
        opt = Optimizer(get_decoder(cfg), cfg)
        args = [np.array(obj[k], np.float32, copy=True) for k in ("t_cam_obj_init", "pts", "rays", "depth")]
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):                # the reference prints its own timing line
            opt.reconstruct_object(args[0].copy(), args[1][:200].copy(), args[2][:200].copy(), args[3][:200].copy())   # warm-up
            t1 = time.perf_counter()
            opt.reconstruct_object(*args)
        return time.perf_counter() - t1
    except Exception as e:
        sys.stderr.write("reference cpu baseline unavailable: %r\n" % (e,))
        return None


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, packed, D):
    """Write the packed result rows (distributed.pack_results: n x 82 float32, every rank's objects in order) as the arrays a caller of the
    batch receives.  Above DUMP_MAX_BYTES a fixed, seeded sample of the objects is kept and its indices go to object_index.npy."""
    packed = np.asarray(packed, np.float32)
    if packed.nbytes > DUMP_MAX_BYTES:
        per_object = packed.itemsize * packed.shape[1] + 8        # its row + its float64 index
        keep = np.sort(np.random.default_rng(0).choice(len(packed), DUMP_MAX_BYTES // per_object, replace=False))
        packed = packed[keep]
    else:
        keep = None
    os.makedirs(out_dir, exist_ok=True)
    t, code, loss, status = D.unpack_results(packed)
    arrays = {"t_cam_obj": t, "code": code, "loss": loss, "status": status}
    if keep is not None:
        arrays["object_index"] = keep.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", choices=("cfg2x64", "cfg4", "cfg5"), default="cfg2x64")
    ap.add_argument("--objects-per-gpu", type=int, default=0)   # 0 = the config's own size
    ap.add_argument("--total-objects", type=int, default=1024)  # cfg4: the fixed job size (strong scaling)
    ap.add_argument("--partition", choices=("static", "measured"), default="static")   # cfg4: object costs for distributed.shard_objects
    ap.add_argument("--prepass", choices=sorted(PREPASS), default="auto")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prepass-off", action="store_true")     # skip the prepass-off sub-record
    ap.add_argument("--no-lp", action="store_true")              # skip the low-precision-compute sub-record (value_lp)
    ap.add_argument("--latency-runs", type=int, default=9)
    ap.add_argument("--serial-batches", action="store_true")     # cfg5: run the two decoders' batches back to back from one host thread (round 5's form)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None)  # the last timed step's results as DIR/<name>.npy (module docstring)
    ap.add_argument("--full", action="store_true")                # also run every leg beyond the headline (module docstring)
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def main():
    args = parse_args()

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus %d needs: python -m torch.distributed.run --nproc-per-node %d bench.py ..." % (args.gpus, args.gpus))
        raise SystemExit("WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no HIP device visible)")
    # Plumbing test only (tests/test_gpu_examples.py): DSP_BENCH_SHARE_GPU=1 puts every rank on device 0 and DSP_BENCH_BACKEND=gloo carries
    # the gather on host tensors, so that the `torch.distributed.run --nproc-per-node N` launch path (rendezvous, per-rank shards, the
    # build lock, gather order, max-over-ranks timing) can be exercised on a ONE-GPU box.  Numbers from such a run mean nothing.
    share_gpu = os.environ.get("DSP_BENCH_SHARE_GPU") == "1"
    backend = os.environ.get("DSP_BENCH_BACKEND", "nccl")
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or os.environ.get("DSP_BENCH_FORCE_DIST") == "1":   # the env switch exercises the RCCL path on one GPU
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # this pool's host driver only supports dmabuf IPC (RCCL needs it across processes)
        os.environ.setdefault("MASTER_PORT", "29533")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    coll_device = torch.device("cuda", local_rank) if backend == "nccl" else torch.device("cpu")

    from dsp_slam_amd import fixtures, synth, engine as E, distributed as D
    from dsp_slam_amd.deep_sdf.deep_sdf_decoder import fold_weight_norm

    sd = fixtures.load_decoder_npz(fixtures.fixture_path("cars"))
    layers = fold_weight_norm(sd, len(fixtures.SPECS["NetworkSpecs"]["dims"]) + 1)
    lat_in, code_len = fixtures.SPECS["NetworkSpecs"]["latent_in"], fixtures.SPECS["CodeLength"]
    eng = E.Engine(layers, lat_in, code_len, device=local_rank)
    engines = [eng]

    # ---- workload -------------------------------------------------------------------------------------------------------
    if args.config == "cfg2x64":
        B = args.objects_per_gpu or 64
        prm = E.gn_params()      # KITTI hyper-parameters (configs/config_kitti.json:21-40 of the reference)
        shards = [(r * B, (r + 1) * B) for r in range(world)]
        objs = synth.make_batch(B, first_seed=1 + rank * B, n_surface=2000, n_background=500)
        groups = [(eng, objs)]
        workload = ("cfg2: single KITTI-like car per object -- 2000 surface pts + 500 free-space rays (2500 rays x 50 depth "
                    "samples), 64-D code, 10 joint GN iterations (Optimizer.reconstruct_object), batch of %d objects per GPU" % B)
    elif args.config == "cfg4":
        # BASELINE configs[3]: a FIXED job of 1024 objects sharded over the GPUs (strong scaling); --objects-per-gpu N makes it N x world (weak)
        total = args.objects_per_gpu * world if args.objects_per_gpu else args.total_objects
        strong = not args.objects_per_gpu
        prm = E.gn_params()
        # Partition: the static cost R*D + 2M by default -- for a list of same-sized objects that is equal counts, which the one-GPU experiment
        # with 8 simulated shards (profiles/r05_cfg4_balance.md) shows balanced to 1.2 % (slowest / mean 1.012): the work of an object is
        # driven by its kept-row count K summed over the TEN iterations, of which a one-iteration measurement predicts only half the
        # variance (correlation 0.51), so --partition measured (every rank measures its equal-count slice with one GN iteration, costs
        # all-gathered, distributed.measure_costs) is for lists whose objects differ in SIZE, not for this one (it measured 1.051 here)
        sa, sb = rank * total // world, (rank + 1) * total // world
        made = {i: synth.make_object(1 + i, n_surface=2000, n_background=500) for i in range(sa, sb)}
        if args.partition == "measured":
            mine_costs = D.measure_costs(eng, prm, [made[i] for i in range(sa, sb)])
            if dist is not None:
                n_max = -(-total // world)
                tt = torch.zeros(n_max, dtype=torch.float64, device=coll_device)
                tt[:len(mine_costs)] = torch.tensor(mine_costs, dtype=torch.float64)
                allc = [torch.empty_like(tt) for _ in range(world)]
                dist.all_gather(allc, tt)
                costs = []
                for r in range(world):
                    costs += [float(x) for x in allc[r][:(r + 1) * total // world - r * total // world].tolist()]
            else:
                costs = mine_costs
        else:
            costs = [D.object_cost(2000, 2500)] * total
        shards = D.shard_objects(costs, world)            # uneven shards are padded in the gather
        a, b = shards[rank]
        objs = [made[i] if i in made else synth.make_object(1 + i, n_surface=2000, n_background=500) for i in range(a, b)]
        del made
        B = b - a
        groups = [(eng, objs)]
        workload = ("cfg4: %d cfg2 objects block-sharded over %d GPU(s) by %s cost (distributed.shard_objects: shards %s), one RCCL gather of "
                    "codes + poses per step" % (total, world, args.partition, [y - x for x, y in shards]))
    else:
        half = (args.objects_per_gpu or 64) // 2
        B = 2 * half
        prm = E.gn_params(**REDWOOD)
        shards = [(r * B, (r + 1) * B) for r in range(world)]
        # second resident decoder: the chairs32 fixture -- 32-D codes (the Redwood chairs option of LocalMapping_util.cc:415-423), its own
        # weights, fitted to a different (taller) shape family
        sd2 = fixtures.load_decoder_npz(fixtures.fixture_path("chairs32"))
        sp2 = fixtures.fixture_specs("chairs32")
        eng2 = E.Engine(fold_weight_norm(sd2, len(sp2["NetworkSpecs"]["dims"]) + 1), sp2["NetworkSpecs"]["latent_in"], sp2["CodeLength"], device=local_rank)
        engines.append(eng2)
        cars = synth.make_batch(half, first_seed=1 + rank * B, n_surface=4000, n_background=500)
        others = [synth.make_object(1 + rank * B + half + i, n_surface=4000, n_background=500, code_len=32, half=synth.CHAIR_HALF) for i in range(half)]
        groups = [(eng, cars), (eng2, others)]
        objs = cars
        workload = ("cfg5: 4000 surface pts + 500 free-space rays x 50 samples, Redwood hyper-parameters (5 iterations), mixed batch on two "
                    "resident decoders (cars: 64-D codes; chairs32: 32-D codes, own weights), %d + %d objects per GPU" % (half, half))
    batches = []
    for e, ol in groups:
        bt = e.batch(prm, [o["t_cam_obj_init"] for o in ol], [o["pts"] for o in ol], [o["rays"] for o in ol], [o["depth"] for o in ol])
        bt.set_prepass(PREPASS[args.prepass])
        bt.set_kernel_timing(1)        # the roofline below is computed from HIP events around every decoder launch
        batches.append(bt)

    gathered = [None]

    # Legs of this process, for matching against `rocprofv3 --kernel-trace` of the same command (tools/rocpd_legs.py): every leg starts with ONE
    # launch of a marker kernel nothing else in this file runs (k_debug_lie through dsp_debug_lie, ~10 us, always outside the timed regions),
    # so a trace splits into the same legs by the marker's dispatches alone; per leg the HIP-event totals of the decoder kernels are kept.
    legs = []

    def mark(name):
        eng.debug_lie(0, np.zeros(7, np.float32))
        legs.append({"leg": name, "fwd_fp32": {"launches": 0, "ms": 0.0}, "prepass": {"launches": 0, "ms": 0.0}, "jacobian": {"launches": 0, "ms": 0.0}})

    def leg_add(st):
        if not legs:
            return
        for key, n, ms in (("fwd_fp32", "n_mlp_fwd_launches", "ms_mlp_fwd"), ("prepass", "n_mlp_prepass_launches", "ms_mlp_prepass"),
                           ("jacobian", "n_mlp_jac_launches", "ms_mlp_jac")):
            legs[-1][key]["launches"] += int(st[n])
            legs[-1][key]["ms"] += float(st[ms])

    # cfg5 holds TWO resident batches (one per decoder = one per handle = one per HIP stream).  Run from one host thread they execute back to back
    # and each pays its own partial rounds and launch tails; run from two host threads (ctypes releases the GIL inside dsp_batch_run) the two
    # streams' kernels interleave on the device ("group objects by decoder").  Results do not depend on it.
    pool = None
    if len(batches) > 1 and not args.serial_batches:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=len(batches))

    def step():
        if pool is not None:
            list(pool.map(lambda bt: bt.run(), batches))
            for bt in batches:
                leg_add(bt.stats())
        else:
            for bt in batches:
                bt.run()
                leg_add(bt.stats())
        if dist is not None and backend == "nccl":     # the single collective of the path: results device -> RCCL gather over xGMI -> rank 0's host, no host bounce
            gathered[0] = D.gather_results_device(batches, shards, dist, device=torch.device("cuda", local_rank))
        elif dist is not None:                         # plumbing test on gloo: host rows
            gathered[0] = D.gather_results(np.concatenate([D.pack_results(*bt.results()) for bt in batches], 0), shards, dist)
        else:
            gathered[0] = np.concatenate([D.pack_results(*bt.results()) for bt in batches], 0)

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    NOT_SUMMED = ("prepass_mode", "prepass_delta", "prepass_max_err", "prepass_guard_max_err")

    def timed(n_warm, n_steps, leg):
        """n_warm untimed + exactly n_steps timed steps, barrier + synchronize on both sides, MAX over ranks.
        -> (elapsed of the slowest rank, every rank's own elapsed, summed kernel stats of this rank)"""
        mark(leg + "_warmup")
        for _ in range(n_warm):
            step()
        mark(leg + "_timed")
        sync()
        t0 = time.perf_counter()
        acc = {}
        for _ in range(n_steps):
            step()
            for bt in batches:
                st = bt.stats()
                for k, v in st.items():
                    acc[k] = (acc.get(k, 0.0) + v) if k not in NOT_SUMMED else max(acc.get(k, 0.0), v)
        own = time.perf_counter() - t0      # this rank's own time for its steps (before the closing barrier): shows imbalance
        sync()
        elapsed = time.perf_counter() - t0
        per_rank = [own]
        if dist is not None:
            tt = torch.tensor([elapsed, own], dtype=torch.float64, device=coll_device)
            allt = [torch.empty_like(tt) for _ in range(world)]
            dist.all_gather(allt, tt)
            elapsed = max(float(x[0].item()) for x in allt)
            per_rank = [float(x[1].item()) for x in allt]
        return elapsed, per_rank, acc

    elapsed, per_rank_s, acc = timed(args.warmup, args.steps, "headline")
    if args.dump_outputs and rank == 0:      # before the legs below overwrite `gathered`; outside every timed region
        dump_outputs(args.dump_outputs, gathered[0], D)
    # the same batch with the prepass OFF, timed in the same run (every rank takes part: the steps contain the collective)
    off_run = None
    if args.full and args.config == "cfg2x64" and int(acc.get("prepass_mode", 0)) != 0 and not args.no_prepass_off:
        for bt in batches:
            bt.set_prepass(0)
        off_steps = max(1, args.steps)        # the strict reference-precision leg is timed over as many steps as the headline
        off_run = timed(1, off_steps, "prepass_off") + (off_steps,)
        for bt in batches:
            bt.set_prepass(PREPASS[args.prepass])
    n_good = int(sum(int((bt.results()[3] == 0).sum()) for bt in batches))
    n_total = sum(b - a for a, b in shards)
    # the same batch in the OPT-IN low-precision compute mode (dsp_batch_set_compute(F16): 16-bit MFMA operands, fp32 accumulation, everywhere in
    # the decoder -- a non-parity fast path, reported separately and never mixed into the fp32 figures), timed in the same run
    lp_run = None
    if args.full and args.config == "cfg2x64" and not args.no_lp:
        try:
            for bt in batches:
                bt.set_compute(1)
            lp_steps = max(1, args.steps)
            lp_run = timed(1, lp_steps, "lp_compute") + (lp_steps, int(sum(int((bt.results()[3] == 0).sum()) for bt in batches)),
                                                          [np.array(x, copy=True) for x in D.unpack_results(gathered[0])] if rank == 0 and gathered[0] is not None else None)
        except Exception as e:
            sys.stderr.write("low-precision compute leg failed: %r\n" % (e,))
            lp_run = None
        for bt in batches:
            bt.set_compute(0)
        mark("restore_fp32_results")
        step()             # leaves the fp32 results in `gathered` for what follows

    # what every rank measured on its own GPU, gathered so that an imbalance in a multi-GPU run is explainable from the line alone:
    # fp32 forward / jacobian / prepass rates (HIP events on the library's stream), the shader clock the chip granted under the
    # prepass kernel, and what the prepass guard saw
    def rank_clock_mhz():
        try:
            import ctypes as C
            from dsp_slam_amd import _lib as L
            lib = L.load()
            lib.dsp_debug_last_clocks.restype = C.c_int
            lib.dsp_debug_last_clocks.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            rngp = np.random.default_rng(0)
            ppts = rngp.uniform(-0.6, 0.6, size=(128 * 256 * 24, 3)).astype(np.float32)
            pcode = np.zeros(64, np.float32)
            mhz = []
            for _ in range(6):
                eng.decode_sdf_prepass(pcode, ppts, 1 if int(acc.get("prepass_mode", 0)) == 1 else 2)
                clk = (C.c_uint64 * 4)()
                L.check(lib.dsp_debug_last_clocks(eng._h, clk), eng._h, "clk")
                mhz.append((clk[2] - clk[0]) / ((clk[3] - clk[1]) / 100e6) / 1e6)
            return float(np.median(mhz[1:]))
        except Exception as e:
            sys.stderr.write("clock probe failed: %r\n" % (e,))
            return 0.0

    def rate(pts, flop, ms):
        return pts * flop / (ms * 1e-3) / 1e12 if ms > 0 else 0.0

    my_clock = 0.0
    if args.full:
        mark("clock_probe")
        my_clock = rank_clock_mhz() if int(acc.get("prepass_mode", 0)) else 0.0
    mine_rec = [rate(acc["n_fwd_points"], F_FWD, acc["ms_mlp_fwd"]),
                (acc["n_jac_points"] * F_JAC + acc["n_render_rows"] * (F_JAC - F_FWD)) / (acc["ms_mlp_jac"] * 1e-3) / 1e12 if acc["ms_mlp_jac"] > 0 else 0.0,
                rate(acc["n_prepass_points"], F_FWD, acc["ms_mlp_prepass"]), my_clock, acc.get("prepass_guard_trips", 0.0),
                acc.get("prepass_guard_rerun", 0.0), acc.get("prepass_guard_max_err", 0.0), float(n_good),
                float(sum(bt.n for bt in batches)), acc["n_insphere_points"] / max(args.steps, 1), acc["n_render_rows"] / max(args.steps, 1),
                acc["ms_mlp_fwd"] / max(args.steps, 1), acc["ms_mlp_jac"] / max(args.steps, 1), acc["ms_mlp_prepass"] / max(args.steps, 1)]
    all_recs = [mine_rec]
    if dist is not None:
        tt = torch.tensor(mine_rec, dtype=torch.float64, device=coll_device)
        allt = [torch.empty_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)
        all_recs = [[float(v) for v in x.tolist()] for x in allt]
        n_good = int(sum(r[7] for r in all_recs))

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    value = n_total * args.steps / elapsed
    # fabric bytes per decoded point from the last committed rocprofv3 --pmc pass (tools/rocpd_pmc.py, FETCH_SIZE x 2 on gfx950)
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    pmc = json.load(open(pmc_path)) if os.path.exists(pmc_path) else {}
    fwd_ms, jac_ms, lp_ms = acc["ms_mlp_fwd"], acc["ms_mlp_jac"], acc["ms_mlp_prepass"]
    fwd_pts, jac_pts, ren_rows, lp_pts = acc["n_fwd_points"], acc["n_jac_points"], acc["n_render_rows"], acc["n_prepass_points"]
    n_fwd, n_jac, n_lp = acc["n_mlp_fwd_launches"], acc["n_mlp_jac_launches"], acc["n_mlp_prepass_launches"]
    insphere_pts = acc["n_insphere_points"]
    fwd_tflops = fwd_pts * F_FWD / (fwd_ms * 1e-3) / 1e12 if fwd_ms > 0 else 0.0
    lp_tflops = lp_pts * F_FWD / (lp_ms * 1e-3) / 1e12 if lp_ms > 0 else 0.0
    # surface points run forward + backward; render rows only the backward sweep (masks come from the forward launches)
    jac_flop = jac_pts * F_JAC + ren_rows * (F_JAC - F_FWD)
    jac_tflops = jac_flop / (jac_ms * 1e-3) / 1e12 if jac_ms > 0 else 0.0
    mode = int(acc.get("prepass_mode", 0))

    def reference_algorithmic(a, seconds):
        """the FLOPs the REFERENCE'S algorithm spends on the same objects -- every in-sphere sample decoded forward (V), every surface
        point and kept render row forward + backward (M + K) -- over this run's wall time.  The timed kernels deliberately do LESS (exact early
        ray termination; with the prepass on most samples are only classified in f16): a ratio above 1 of the fp32 peak says so in the line itself."""
        # dsp_stats: with mask reuse n_jac_points = sum of M and n_render_rows = sum of K; without, n_jac_points = sum of M + K and n_render_rows = 0
        flop = a["n_insphere_points"] * F_FWD + (a["n_jac_points"] + a["n_render_rows"]) * F_JAC
        tf = flop / seconds / 1e12 * world
        return {"reference_algorithmic_flop_per_step": round(flop / max(args.steps, 1)), "reference_algorithmic_tflops": round(tf, 1),
                "reference_algorithmic_over_fp32_peak": round(tf / (PEAK_FP32_MFMA_TFLOPS * world), 3)}

    result = {
        "metric": {"cfg2x64": "objects/sec (2000 pts, 64-D code, 10 GN iters)", "cfg4": "objects/sec (2000 pts, 64-D code, 10 GN iters; 1024-object job sharded over the GPUs)",
                   "cfg5": "objects/sec (4000 pts, 64-D + 32-D codes on two decoders, 5 GN iters, Redwood hyper-parameters)"}[args.config],
        "value": round(value, 3),
        "unit": "objects/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "full": args.full,          # False: the headline leg alone; True: every leg of the module docstring
        "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "ms_per_step_by_rank": [round(x / args.steps * 1e3, 3) for x in per_rank_s],
        "by_rank": [{"rank": r, "fwd_fp32_frac": round(x[0] / PEAK_FP32_MFMA_TFLOPS, 4), "jac_fp32_frac": round(x[1] / PEAK_FP32_MFMA_TFLOPS, 4),
                     "prepass_tflops": round(x[2], 1), "prepass_clock_mhz": round(x[3]) if x[3] > 0 else None, "guard_trips": x[4], "guard_reruns": x[5],
                     "guard_max_err": x[6], "objects_good": int(x[7]), "objects": int(x[8]), "sum_V_per_step": round(x[9]), "sum_K_per_step": round(x[10]),
                     "ms_per_step_by_kernel": {"fwd_fp32": round(x[11], 2), "jacobian_fp32": round(x[12], 2), "prepass": round(x[13], 2)}}
                    for r, x in enumerate(all_recs)],
        "higher_is_better": True,
        "scaling": "strong" if (args.config == "cfg4" and not args.objects_per_gpu) else "weak",
        "vs_baseline": None,
        # what computed: every result-bearing value in fp32 (v_mfma_f32_16x16x4_f32); with the prepass on, an f16 MFMA kernel additionally
        # CLASSIFIES ray samples whose occupancy is exactly 0 or 1 (results bit-identical to the fp32-only run, value_fp32_only below)
        "dtype": "f32 + f16 classifier" if mode == 1 else ("f32 + bf16 classifier" if mode == 2 else "f32"),
        "value_fp32_only": None,      # objects/s of the same batch with the prepass off (every sample the reference decodes, decoded in fp32): filled below (with the prepass on: --full only)
        "data": "synthetic (seeded rounded-box objects, decoder fixture fitted to them; no real weights/datasets offline)",
        "config": {
            "workload": workload,
            "name": args.config,
            "objects_per_gpu": B,
            "objects_good": n_good,
            "timed_region": "inputs are resident in HBM before the timed step (dsp_batch_create uploaded them: ~4 MB per 64 objects, ~0.1 ms over PCIe, NOT "
                            "in the step); the step = every GN iteration on the device + the read-back of the 82-float result rows + the gather",
            "parallelism": "object-sharded x%d, one RCCL gather of results per step" % world + (" [PLUMBING TEST: ranks share GPU 0, %s backend]" % backend if share_gpu else "") + (
                "; the %d decoders' batches run concurrently on their own HIP streams (one host thread each)" % len(batches) if pool is not None else ""),
            "prepass": ["off", "f16", "bf16"][mode] + (" (exact pre-classification of ray samples; results bit-identical to off)" if mode else ""),
        },
        "roofline": {
            "bound": "mfma",
            "kernel": "mlp_kernel<1,false> (decoder forward with relu-mask export, fp32 v_mfma_f32_16x16x4_f32)",
            "achieved": round(fwd_tflops, 2),
            "peak": PEAK_FP32_MFMA_TFLOPS,
            "unit": "TFLOP/s",
            "frac": round(fwd_tflops / PEAK_FP32_MFMA_TFLOPS, 4),
            "traffic": pmc.get("fwd_fetch_bytes_per_point", 0.0) * fwd_pts / max(n_fwd, 1) or None,
            "traffic_note": pmc.get("note", "no PMC pass recorded (profiles/pmc_traffic.json missing)"),
            "avg_launch_ms": round(fwd_ms / max(n_fwd, 1), 4),
            # what `rocprofv3 --kernel-trace` of THIS command must show, leg by leg (filled at the end: tools/rocpd_legs.py splits the trace by the
            # marker kernel's dispatches and compares every leg's launch count and average duration with these HIP-event figures)
            "rocprof_check": None,
            "alg_flop_per_launch": round(fwd_pts * F_FWD / max(n_fwd, 1)),
            "fwd_points_evaluated_over_insphere": round(fwd_pts / max(insphere_pts, 1.0), 4),
            "render_rows_kept_over_fwd_points": round(ren_rows / max(fwd_pts, 1.0), 4),
            "jac_kernel_tflops": round(jac_tflops, 2),
            "jac_kernel_frac": round(jac_tflops / PEAK_FP32_MFMA_TFLOPS, 4),
            "jac_avg_launch_ms": round(jac_ms / max(n_jac, 1), 4),
            "whole_path_fp32_tflops": round((fwd_pts * F_FWD + jac_flop) / elapsed / 1e12 * world, 2),
            **reference_algorithmic(acc, elapsed),
            "reference_algorithmic_note": "SURVEY 8(d) formula: sum V x 3.671 MFLOP + (sum M + sum K) x 7.342 MFLOP over the step time.  Above 1.0 of the fp32 MFMA peak = work the "
                                          "reference does that is provably skipped here, result-neutral (exact early ray termination: samples behind a ray's first solid sample; f16 "
                                          "classification of samples whose occupancy is exactly 0 or 1: tests test_early_ray_termination_is_exact, test_prepass_is_exact_*)",
            "ms_per_step_by_kernel": {"prepass": round(lp_ms / args.steps, 2), "fwd_fp32": round(fwd_ms / args.steps, 2),
                                      "jacobian_fp32": round(jac_ms / args.steps, 2),
                                      "other": round((acc["ms_total"] - lp_ms - fwd_ms - jac_ms) / args.steps, 2)},
        },
    }
    if mode:
        result["prepass"] = {
            "bound": "mfma",
            "kernel": "mlp_lp_kernel<%s> (decoder forward, v_mfma_f32_16x16x32_%s, classification only)" % (("false", "f16") if mode == 1 else ("true", "bf16")),
            "dtype": "f16" if mode == 1 else "bf16",
            "achieved": round(lp_tflops, 1),
            "peak": PEAK_16BIT_MFMA_TFLOPS,
            "unit": "TFLOP/s",
            "frac": round(lp_tflops / PEAK_16BIT_MFMA_TFLOPS, 4),
            "avg_launch_ms": round(lp_ms / max(n_lp, 1), 4),
            "alg_flop_per_launch": round(lp_pts * F_FWD / max(n_lp, 1)),
            "points_over_insphere": round(lp_pts / max(insphere_pts, 1.0), 4),
            "delta": acc.get("prepass_delta"),
            "traffic": pmc.get("lp_fetch_bytes_per_point", 0.0) * lp_pts / max(n_lp, 1) or None,
        }

    if mode:
        # the clock the chip grants under this kernel (dense 16-bit MFMA): shader cycles / wall ticks of workgroup 0 of a bare prepass decode (rank 0's)
        clk_mhz = all_recs[0][3]
        if clk_mhz > 0:
            result["prepass"]["sustained_clock_mhz"] = round(clk_mhz)
            result["prepass"]["frac_of_peak_at_sustained_clock"] = round(lp_tflops / (PEAK_16BIT_MFMA_TFLOPS * clk_mhz / 2400.0), 4)
            result["prepass"]["clock_note"] = ("the chip holds this clock under dense 16-bit MFMA while drawing LESS socket power than under the fp32 kernel at 2.37 GHz "
                                               "(profiles/r03_power_probe.md); DESIGN.md K0")
        else:
            result["prepass"]["sustained_clock_mhz"] = None
    if mode:
        result["prepass"]["guard"] = {"trips": acc.get("prepass_guard_trips", 0.0), "reruns": acc.get("prepass_guard_rerun", 0.0),
                                      "max_err_seen": acc.get("prepass_guard_max_err", 0.0),
                                      "note": "always on: the fp32 kernel compares every sample it re-decodes (the whole widened band + 1/8 of the ring beyond it + 1/512 of the rest) with the prepass value"}
    if off_run is not None:
        o_el, o_ranks, o_acc, o_steps = off_run
        o_tf = o_acc["n_fwd_points"] * F_FWD / (o_acc["ms_mlp_fwd"] * 1e-3) / 1e12 if o_acc["ms_mlp_fwd"] > 0 else 0.0
        o_jflop = o_acc["n_jac_points"] * F_JAC + o_acc["n_render_rows"] * (F_JAC - F_FWD)
        result["prepass_off"] = {
            "value": round(n_total * o_steps / o_el, 3), "unit": "objects/s", "steps": o_steps, "ms_per_step": round(o_el / o_steps * 1e3, 3),
            "roofline_frac": round(o_tf / PEAK_FP32_MFMA_TFLOPS, 4), "fwd_fp32_tflops": round(o_tf, 2),
            "fwd_avg_launch_ms": round(o_acc["ms_mlp_fwd"] / max(o_acc["n_mlp_fwd_launches"], 1), 4),
            "jac_kernel_frac": round(o_jflop / (o_acc["ms_mlp_jac"] * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4) if o_acc["ms_mlp_jac"] > 0 else None,
            "whole_path_fp32_tflops": round((o_acc["n_fwd_points"] * F_FWD + o_jflop) / o_el / 1e12 * world, 2),
            **{k: v for k, v in reference_algorithmic(o_acc, o_el).items() if k != "reference_algorithmic_flop_per_step"},
            "note": "same batch, same process, prepass off: every sample in front of a ray's first solid sample decoded by the fp32 kernel; results bit-identical to the headline run",
        }
        result["value_fp32_only"] = result["prepass_off"]["value"]
    elif mode == 0:
        result["value_fp32_only"] = result["value"]
    result["value_lp"] = None
    if lp_run is not None:
        l_el, l_ranks, l_acc, l_steps, l_good, l_res = lp_run
        PEAK_LIVE = 1781.0       # profiles/r05_k0_clock.md row F: what a 16x16x32 f16 MFMA stream with live operands and one A-fragment read per two MFMAs sustains
        lj_tf = l_acc["n_jac_points"] * F_JAC / (l_acc["ms_mlp_jac"] * 1e-3) / 1e12 if l_acc["ms_mlp_jac"] > 0 else 0.0
        lf_tf = l_acc["n_prepass_points"] * F_FWD / (l_acc["ms_mlp_prepass"] * 1e-3) / 1e12 if l_acc["ms_mlp_prepass"] > 0 else 0.0
        fp32_res = D.unpack_results(gathered[0])
        lp_block = {
            "value": round(n_total * l_steps / l_el, 3), "unit": "objects/s", "steps": l_steps, "ms_per_step": round(l_el / l_steps * 1e3, 3),
            "dtype": "f16 operands, f32 accumulation (v_mfma_f32_16x16x32_f16) in every decoder launch; thresholds, scans, Gram and the fp64 solve unchanged",
            "parity": "NOT the parity path (opt-in: dsp_batch_set_compute): accuracy at the reference's recorded states in profiles/r06_lp_compute.md / tests/test_gpu_lp_compute.py",
            "objects_good": l_good,
            "vs_value": round((n_total * l_steps / l_el) / value, 3),
            "roofline": {
                "bound": "mfma", "peak": PEAK_16BIT_MFMA_TFLOPS, "unit": "TFLOP/s",
                "jacobian": {"kernel": "mlp_lpj_fwd_kernel<f16> + mlp_lpj_bwd_kernel<f16> (forward with relu-mask export, backward over the transposed stream)",
                             "achieved": round(lj_tf, 1), "frac": round(lj_tf / PEAK_16BIT_MFMA_TFLOPS, 4), "frac_of_live_operand_ceiling": round(lj_tf / PEAK_LIVE, 4),
                             "alg_flop_per_launch_pair": round(l_acc["n_jac_points"] * F_JAC / max(l_acc["n_mlp_jac_launches"], 1)),
                             "avg_launch_pair_ms": round(l_acc["ms_mlp_jac"] / max(l_acc["n_mlp_jac_launches"], 1), 4)},
                "ray_samples": {"kernel": "mlp_lp_kernel<f16> (the prepass kernel: here its values ARE the samples' sdf)", "achieved": round(lf_tf, 1),
                                "frac": round(lf_tf / PEAK_16BIT_MFMA_TFLOPS, 4), "frac_of_live_operand_ceiling": round(lf_tf / PEAK_LIVE, 4),
                                "avg_launch_ms": round(l_acc["ms_mlp_prepass"] / max(l_acc["n_mlp_prepass_launches"], 1), 4)},
                "live_operand_ceiling_tflops": PEAK_LIVE,
                "ms_per_step_by_kernel": {"ray_samples_f16": round(l_acc["ms_mlp_prepass"] / l_steps, 2), "jacobian_f16": round(l_acc["ms_mlp_jac"] / l_steps, 2),
                                          "fwd_fp32": round(l_acc["ms_mlp_fwd"] / l_steps, 2),
                                          "other": round((l_acc["ms_total"] - l_acc["ms_mlp_prepass"] - l_acc["ms_mlp_jac"] - l_acc["ms_mlp_fwd"]) / l_steps, 2)},
            },
            **{k: v for k, v in reference_algorithmic(l_acc, l_el).items() if k != "reference_algorithmic_flop_per_step"},
        }
        if l_res is not None:       # how far this run's results sit from the fp32 path's, object by object (chained over ten iterations: includes the map's own amplification)
            t_lp, c_lp, t_32, c_32 = l_res[0], l_res[1], fp32_res[0], fp32_res[1]
            dtr = np.abs(t_lp - t_32).reshape(len(t_lp), -1).max(1) / np.abs(t_32).reshape(len(t_32), -1).max(1)
            dcd = np.abs(c_lp - c_32).max(1)
            lp_block["chained_result_vs_fp32_path"] = {"pose_rel_median": float(np.median(dtr)), "pose_rel_max": float(dtr.max()), "code_abs_median": float(np.median(dcd)),
                                                       "code_abs_max": float(dcd.max()),
                                                       "note": "for scale: the unmodified reference moves these objects by 2e-4 .. 2e-2 (pose) when its inputs move by one float32 ulp or its thread count changes (tests/golden/golden_bench_cfg2x64.npz)"}
        result["lp_compute"] = lp_block
        result["value_lp"] = lp_block["value"]

    if args.full and world == 1 and args.config == "cfg2x64":
        # single-object latency (ms/object p50): batch of ONE cfg2 object
        o = objs[0]
        one = eng.batch(prm, [o["t_cam_obj_init"]], [o["pts"]], [o["rays"]], [o["depth"]])
        one.set_prepass(PREPASS[args.prepass])
        mark("latency_cfg2_object")
        one.run()
        leg_add(one.stats())
        lat = []
        for _ in range(max(args.latency_runs, 1)):
            t1 = time.perf_counter()
            one.run()
            one.results()
            lat.append((time.perf_counter() - t1) * 1e3)
            leg_add(one.stats())
        result["latency_ms_p50"] = round(statistics.median(lat), 3)
        if result.get("lp_compute") is not None:     # the same object in the opt-in low-precision compute mode (a non-parity figure: kept inside that block)
            one.set_compute(1)
            mark("latency_cfg2_object_lp_compute")
            one.run()
            lat = []
            for _ in range(max(args.latency_runs, 1)):
                t1 = time.perf_counter()
                one.run()
                one.results()
                lat.append((time.perf_counter() - t1) * 1e3)
            result["lp_compute"]["latency_cfg2_object_ms_p50"] = round(statistics.median(lat), 3)
            result["lp_compute"]["latency_note"] = ("one cfg2 object, resident batch, p50 as latency_ms_p50; a detection of SLAM's real size keeps the fp32 latency path with the mode set "
                                                    "(faster there: profiles/r06_latency_ab.md), so latency_kitti_size_ms_p50 is the same in both modes")
        one.close()
        # a detection of the reference's real KITTI size (config_kitti.json:17 num_lidar_max 250, kitti_sequence.py:203-205 <= 200 background rays)
        k = synth.make_object(4242, n_surface=250, n_background=200)
        one = eng.batch(prm, [k["t_cam_obj_init"]], [k["pts"]], [k["rays"]], [k["depth"]])
        one.set_prepass(PREPASS[args.prepass])
        mark("latency_kitti_size_detection")
        one.run()
        leg_add(one.stats())
        lat = []
        for _ in range(max(args.latency_runs, 1)):
            t1 = time.perf_counter()
            one.run()
            one.results()
            lat.append((time.perf_counter() - t1) * 1e3)
            leg_add(one.stats())
        one.close()
        result["latency_kitti_size_ms_p50"] = round(statistics.median(lat), 3)
        # the call SLAM really makes (Optimizer.reconstruct_object -> dsp_reconstruct_batch: build the batch from host buffers, run, drop): same detection
        args1 = ([k["t_cam_obj_init"]], [k["pts"]], [k["rays"]], [k["depth"]])
        mark("latency_one_shot (launch counts not recorded: the one-shot entry point returns no stats)")
        eng.reconstruct_batch(prm, *args1)
        lat = []
        for _ in range(max(args.latency_runs, 1)):
            t1 = time.perf_counter()
            eng.reconstruct_batch(prm, *args1)
            lat.append((time.perf_counter() - t1) * 1e3)
        result["latency_one_shot_ms_p50"] = round(statistics.median(lat), 3)
        result["latency_note"] = ("ms per object, p50 over %d runs, host wall clock around run + results: latency_ms_p50 = one cfg2 object (2000 + 500 rays), resident batch; "
                                  "latency_kitti_size_ms_p50 = one detection of the reference's real size (250 LiDAR points + 200 background rays, config_kitti.json:17), "
                                  "resident batch; latency_one_shot_ms_p50 = the same detection through the one-shot entry point (host buffers in, PCIe both ways)" % max(args.latency_runs, 1))
        # sdf-only workload: Optimizer.estimate_pose_cam_obj on the same objects -- 5 Gauss-Newton iterations of the
        # surface term alone, through the one-shot entry point (host buffers in, so this figure includes upload and download)
        try:
            t_se3, scales = [], []
            for o in objs:
                t = np.array(o["t_cam_obj_init"], np.float32)
                sc = float(np.cbrt(np.linalg.det(t[:3, :3].astype(np.float64))))
                t[:3, :3] /= sc
                t_se3.append(t); scales.append(sc)
            zero_codes = [np.zeros(64, np.float32)] * len(objs)
            pts_list = [o["pts"] for o in objs]
            mark("pose_only (launch counts not recorded)")
            eng.estimate_pose_batch(prm, t_se3, scales, pts_list, zero_codes)
            t1 = time.perf_counter()
            reps = 5
            for _ in range(reps):
                eng.estimate_pose_batch(prm, t_se3, scales, pts_list, zero_codes)
            dt_pose = (time.perf_counter() - t1) / reps
            result["pose_only"] = {"objects_per_s": round(len(objs) / dt_pose, 1), "ms_per_batch": round(dt_pose * 1e3, 3),
                                   "note": "estimate_pose_cam_obj, %d objects x 2000 points x 5 iterations per call, host buffers in/out" % len(objs)}
        except Exception as e:      # never lose the headline line over the secondary figure
            result["pose_only"] = {"error": repr(e)}

    if args.full and world == 1 and not args.no_cpu_baseline:
        # checker / baseline code only -- never on the product path
        from oracle import dsp_oracle as O, torch_baseline as TB
        oprm = O.GNParams(**(dict(k1=10.0, k2=100.0, k3=2.5, k4=0.0, b1=0.2, b2=0.02, lr=1.0, s_damp=100.0, num_iterations=5) if args.config == "cfg5" else {}))
        tb_dec = TB.build_decoder(sd, fixtures.SPECS)          # parameters keep requires_grad, as the reference leaves them
        # pick the intra-op thread count that runs a small object fastest (128-thread hosts are slower at 128 than at 16-32)
        small = synth.make_object(999, n_surface=500, n_background=0)
        oprm2 = O.GNParams(num_iterations=2)
        ncpu = os.cpu_count() or 1
        best_threads, best_t = None, None
        for nt in sorted({min(ncpu, x) for x in (8, 16, 32, 64, ncpu)}):
            torch.set_num_threads(nt)
            TB.reconstruct_object(tb_dec, oprm2, small["t_cam_obj_init"], small["pts"], small["rays"], small["depth"])
            t1 = time.perf_counter()
            TB.reconstruct_object(tb_dec, oprm2, small["t_cam_obj_init"], small["pts"], small["rays"], small["depth"])
            dt_s = time.perf_counter() - t1
            if best_t is None or dt_s < best_t:
                best_threads, best_t = nt, dt_s
        torch.set_num_threads(best_threads)
        # one warm-up, then >= 3 objects (the bench's first three: seeds 1, 2, 3 on rank 0), objects/s = 1 / mean, p50 reported
        n_base = min(3, len(objs))
        kind = "port"
        use_ref = args.config != "cfg5" and bool(os.environ.get("DSP_REFERENCE_ROOT"))      # never probed unless asked for: the GPU box has no checkout
        TB.reconstruct_object(tb_dec, O.GNParams(num_iterations=1), small["t_cam_obj_init"], small["pts"], small["rays"], small["depth"])     # warm-up at the chosen thread count
        times, times_tb, r = [], [], None
        for o in objs[:n_base]:
            dt = reference_cpu_baseline(o, best_threads) if use_ref else None
            if dt is not None:
                kind = "reference"
            t1 = time.perf_counter()
            ri = TB.reconstruct_object(tb_dec, oprm, o["t_cam_obj_init"], o["pts"], o["rays"], o["depth"])
            dt_tb = time.perf_counter() - t1
            times_tb.append(dt_tb)
            times.append(dt if dt is not None else dt_tb)
            if r is None:
                r = ri
        dt = float(np.mean(times))
        dt_tb = float(np.mean(times_tb))
        cal_path = os.path.join(ROOT, "profiles", "cpu_baseline_calibration.json")
        cal = json.load(open(cal_path)) if os.path.exists(cal_path) else {}
        gpu_t = D.unpack_results(gathered[0])[0][0]
        result["cpu_baseline"] = {
            "value": round(1.0 / dt, 4),
            "unit": "objects/s",
            "cores": int(best_threads),
            "kind": kind,
            "port": None if kind == "reference" else "torch-restatement (oracle/torch_baseline.py: the reference's torch op sequence, bit-identical results, 1.016 x its time)",
            "n_objects": n_base,
            "s_per_object": [round(x, 3) for x in times],
            "s_per_object_p50": round(float(np.median(times)), 3),
            "calibrated_vs_reference": cal.get("torch_baseline_over_reference"),
            "calibration": "profiles/cpu_baseline_calibration.json: oracle/torch_baseline.py takes %s x the unmodified reference's time on the same cfg2 object "
                           "(build container, %s threads), results bit-identical" % (cal.get("torch_baseline_over_reference"), cal.get("threads")),
            "sample": "1 warm-up + %d %s objects (seeds %d..%d), all %d GN iterations each, %s on %d of %d host threads (fastest of a small sweep); value = 1 / mean(%s s)%s" % (
                n_base, "cfg5 (4000-pt)" if args.config == "cfg5" else "cfg2", 1 + rank * B, n_base + rank * B, oprm.num_iterations,
                "the unmodified reference (reconstruct/optimizer.py via oracle/ref_shim.py, torch CPU)" if kind == "reference"
                else "oracle/torch_baseline.py: the reference's torch op sequence restated (weight-normed nn.Linear chain, autograd input gradient with "
                     "parameters requiring grad, bmm Gram, torch.inverse) -- no reference checkout on this box",
                best_threads, ncpu, ", ".join("%.2f" % x for x in times), "; the torch restatement took %.2f s on average" % dt_tb if kind == "reference" else ""),
            "gpu_vs_cpu": round(value * dt, 1),
            "gpu_fp32_only_vs_cpu": round(result["value_fp32_only"] * dt, 1) if result.get("value_fp32_only") else None,
            "pose_max_abs_diff_vs_gpu": float(np.abs(r["t_cam_obj"] - gpu_t).max()) if r["is_good"] else None,
        }
    kernel_of = {"fwd_fp32": "mlp_kernel<1> (+ mlp_split_kernel<1> tail tiles in the one-object legs)", "prepass": "mlp_lp_kernel<f16|bf16>",
                 "jacobian": "mlp_kernel<2> + mlp_kernel<3> (64-object legs) / mlp_cluster_kernel + mlp_split_kernel<2> (one-object legs)"}
    result["roofline"]["rocprof_check"] = {
        "marker_kernel": "k_debug_lie: one dispatch opens every leg, in this order (dispatches before the first marker: dsp_create's prepass calibration)",
        "kernels": kernel_of,
        "note": "avg_ms = HIP-event time on the library's stream / launches; null where the leg runs without per-kernel events (batches of <= 16 objects)",
        "legs": [{"leg": lg["leg"], **{k: {"launches": lg[k]["launches"], "avg_ms": round(lg[k]["ms"] / lg[k]["launches"], 4) if lg[k]["launches"] and lg[k]["ms"] > 0 else None}
                                         for k in ("fwd_fp32", "prepass", "jacobian")}} for lg in legs]}
    for bt in batches:
        bt.close()
    for e in engines:
        e.close()
    if dist is not None:
        dist.destroy_process_group()
    try:    # RCCL prints its banner through C stdio; flush it so that the JSON is the LAST line of stdout
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
