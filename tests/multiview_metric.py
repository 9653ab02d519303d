"""What the multi-view metric tests share (tests/test_multiview_metric.py on the CPU, tests/test_gpu_multiview_metric.py on the device,
tools/measure_gn_metric.py --multiview): the inputs of every case, the composed fp32 oracle (tests/multiview_oracle.py) and its sdf-jitter
twin linearised at one state with the pooled fp64 system (oracle.dsp_oracle.linearise_fp64_multiview) on the oracle's own sets, and the
faults a multi-view implementation could make, built at the level of one view's rows.  Test helper, not a test."""
import numpy as np

import gn_metric as M
import multiview_oracle as MV
from oracle import dsp_oracle as O

F32 = np.float32
EYE = np.eye(4, dtype=F32)
HYPER = dict(k1=1.0, k2=100.0, k3=0.25, k4=1e7, b1=0.2, b2=0.025, lr=1.0, s_damp=1.0)
PD = 7


def oracle_params(case, num_iterations=1):
    return O.GNParams(num_iterations=num_iterations, code_len=case["code_len"], num_depth_samples=case["n_depth"], cut_off=case["cut_off"], **HYPER)


def away_view(o, n_pts=50):
    """A view whose rays all miss the object (V = 0 < 10: no render term) but whose surface points count."""
    return dict(t_ref_cam=EYE, pts=o["pts"][:n_pts], rays=np.tile(np.array([[5.0, 5.0, 1.0]], F32), (30, 1)), depth=np.zeros(0, F32))


def one_view(o):
    return [dict(t_ref_cam=EYE, pts=o["pts"], rays=o["rays"], depth=o["depth"])]


# Seeds: chosen with the composed oracle so that every iteration of its own run selects the same sets as its jitter twin (no sample within
# 2e-7 of a threshold) and, where the case is built for a transition, shows it; tests/test_multiview_metric.py asserts both.
THREE_VIEW_SEED = 31
RAGGED_SEEDS = (41, 42, 43)          # objects of 2, 1 and 3 views
AWAY_SEED = 64
DEPTH_SEED = 52
CHAIRS_SEED = 81


def _case(objects, n_it, decoder="cars", code_len=64, n_depth=50, cut_off=0.01, **extra):
    return dict(objects=objects, n_it=n_it, decoder=decoder, code_len=code_len, n_depth=n_depth, cut_off=cut_off, **extra)


def _mv(seed, **kw):
    from dsp_slam_amd import synth
    o = synth.make_object_multiview(seed, **kw)
    return dict(t=o["t_cam_obj_init"], views=o["views"])


def case_three_views():
    return _case([_mv(THREE_VIEW_SEED, n_views=3, n_surface=120, n_background=40)], 3)


def case_ragged():
    return _case([_mv(s, n_views=nv, n_surface=100, n_background=30) for s, nv in zip(RAGGED_SEEDS, (2, 1, 3))], 2)


def case_late_join():
    t, views = MV.late_join_case()
    return _case([dict(t=t, views=views)], 4, transition="join")


def case_leaving():
    t, views = MV.leaving_case()
    return _case([dict(t=t, views=views)], 5, transition="leave")


def case_away():
    """Object 0: one good view and one away view; object 1: away views only (ends OBJ_FEW_SAMPLES; status 1 in the composed oracle)."""
    from dsp_slam_amd import synth
    o = synth.make_object(AWAY_SEED, n_surface=150, n_background=40)
    return _case([dict(t=o["t_cam_obj_init"], views=one_view(o) + [away_view(o)]), dict(t=o["t_cam_obj_init"], views=[away_view(o), away_view(o)], fails=True)],
                 2, transition="away")


def case_depth(n_depth):
    return _case([_mv(DEPTH_SEED, n_views=2, n_surface=100, n_background=30)], 2, n_depth=n_depth)


def case_chairs32():
    from dsp_slam_amd import synth
    return _case([_mv(CHAIRS_SEED, n_views=2, n_surface=100, n_background=30, code_len=32, half=synth.CHAIR_HALF)], 3, decoder="chairs32", code_len=32)


CASES = {"three_views": case_three_views, "ragged": case_ragged, "late_join": case_late_join, "leaving": case_leaving, "away_view": case_away,
         "depth33": lambda: case_depth(33), "depth64": lambda: case_depth(64), "chairs32": case_chairs32}


def linearise_at(dec, oprm, views, t_obj_cam, code, depths=None, fp64=True):
    """The composed fp32 oracle at (t_obj_cam, code) on the per-view depth samples `depths` (None: its own), its sdf-jitter twin and the
    pooled fp64 system on the first one's sets -> (it, itj, lin), or None where the oracle has no linearisation there."""
    o1 = O.GNParams(oprm.k1, oprm.k2, oprm.k3, oprm.k4, oprm.b1, oprm.b2, oprm.lr, oprm.s_damp, 1, oprm.code_len, oprm.num_depth_samples, oprm.cut_off)
    out = []
    for jit in (0.0, M.SDF_ROUNDOFF):
        tr = []
        MV.reconstruct_object_multiview(dec, o1, None, views, code, trace=tr, t_obj_cam0=t_obj_cam, depths_override=depths, sdf_jitter=jit)
        if not tr:
            return None
        out.append(tr[0])
    it = out[0]
    lin = None
    if fp64:
        lin = O.linearise_fp64_multiview(dec, oprm, views, t_obj_cam, code, [v["depths"] for v in it["views"]], [v["sets"] for v in it["views"]])
        lin["k4"] = oprm.k4
    return it, out[1], lin


def same_sets(it, itj):
    return all((a["V"], a["K"], a["vsum"], a["ksum"]) == (b["V"], b["K"], b["vsum"], b["ksum"]) for a, b in zip(it["views"], itj["views"]))


def own_run(dec, oprm, obj, n_it):
    """Every iteration of the composed oracle's own chained run from the object's start pose -> [(it, itj, lin), ...]."""
    tr = []
    MV.reconstruct_object_multiview(dec, oprm, obj["t"], obj["views"], trace=tr, num_iterations=n_it)
    return [linearise_at(dec, oprm, obj["views"], t["t_obj_cam"], t["code"]) for t in tr]


def view_vk(it):
    return [(v["V"], v["K"]) for v in it["views"]]


def max_norm_passes(sys_, it, k4):
    """The bounds tests/test_gpu_multiview.py holds a pooled system to: |dH| < 1e-4 max|H|; |db| <= 1e-4 max|b|, plus the rotation prior's
    quantisation on entries 3:6."""
    tol_b = np.full(it["b"].shape[0], 1e-4 * np.abs(it["b"]).max())
    tol_b[3:6] += MV.rot_prior_bound(it["H"], k4)
    eh = np.abs(np.asarray(sys_["H"], np.float64) - it["H"]).max() / np.abs(it["H"]).max()
    return bool(eh < 1e-4 and np.all(np.abs(np.asarray(sys_["b"], np.float64) - it["b"]) <= tol_b))


# ---------------------------------------------------------------------------------------------------------------------------------------
# faults
# ---------------------------------------------------------------------------------------------------------------------------------------
def view_rows(dec, oprm, view, info, code):
    """The fp32 oracle's rows of one view at its traced state `info` (a `views` entry of the composed oracle's trace): (J_s, r_s, J_r, r_r)
    with the raw residuals, float64 copies; zero rows where the view has none."""
    n = PD + oprm.code_len
    z = np.asarray(code, F32)[:oprm.code_len]
    pts, rays, depth = (np.asarray(view[k], F32) for k in ("pts", "rays", "depth"))
    j_s, r_s, j_r, r_r = np.zeros((0, n)), np.zeros(0), np.zeros((0, n)), np.zeros(0)
    if pts.shape[0]:
        j7, jc, r = O.compute_sdf_loss(dec, pts, info["t_obj_cam"], z)
        j_s, r_s = np.concatenate([j7, jc], -1).astype(np.float64), r.astype(np.float64)
    if rays.shape[0]:
        d = info["depths"]
        depth_obs = np.concatenate([depth, np.full(rays.shape[0] - depth.shape[0], F32(1.1) * d[-1], F32)]).astype(F32)
        rend = O.compute_render_loss(dec, rays, depth_obs, info["t_obj_cam"], d, z, th=oprm.cut_off)
        if rend is not None:
            j7, jc, r = rend
            j_r, r_r = np.concatenate([j7, jc], -1).astype(np.float64), r.astype(np.float64)
    return j_s, r_s, j_r, r_r


def _data_terms(oprm, rows, n_s=None, n_k=None):
    """(H, b) data parts of the pooled rows [(J_s, r_s, J_r, r_r) per view] in float64; n_s / n_k: the divisors (default: the pooled counts)."""
    j_s, r_s, j_r, r_r = (np.concatenate([r[k] for r in rows]) for k in range(4))
    rr_s = O.get_robust_res(r_s, oprm.b2)[0].astype(np.float64)
    rr_r = O.get_robust_res(r_r, oprm.b1)[0].astype(np.float64)
    n_s = j_s.shape[0] if n_s is None else n_s
    n_k = j_r.shape[0] if n_k is None else n_k
    return oprm.k1 * j_r.T @ j_r / n_k + oprm.k2 * j_s.T @ j_s / n_s, -oprm.k1 * j_r.T @ rr_r / n_k - oprm.k2 * j_s.T @ rr_s / n_s


def _faulty(it, oprm, good, bad, **div):
    """The oracle's fp32 system with its data part moved by (faulty rows' terms - good rows' terms), rounded to fp32, dx re-solved in fp32."""
    h0, b0 = _data_terms(oprm, good)
    h1, b1 = _data_terms(oprm, bad, **div)
    h = (np.asarray(it["H"], np.float64) + h1 - h0).astype(F32)
    b = (np.asarray(it["b"], np.float64) + b1 - b0).astype(F32)
    return dict(H=h, b=b, dx=(np.linalg.inv(h) @ b).astype(F32))


FAULTS = ("view 2: 8 code columns of its render rows missing", "view 1: 8 code columns of its render rows x 1.01", "view 1: decoded with the previous iteration's code",
          "render Gram divided by the leader's K", "view 2: surface jacobian missing, M still pooled", "view 1: last three render rows lost")
MUST_REJECT = FAULTS[:5]


def faults(dec, oprm, views, it, prev_code):
    """{fault: system} -- the six faults of a member view on its way into the leader's sums, at the state of the composed oracle's trace
    entry `it` (an object of at least three views).  prev_code: the code of the iteration before."""
    good = [view_rows(dec, oprm, v, info, it["code"]) for v, info in zip(views, it["views"])]
    n_s, n_k = sum(r[0].shape[0] for r in good), sum(r[2].shape[0] for r in good)
    cols = PD + np.arange(8, 16)                       # eight code columns: one 8-wide fragment

    def swap(v, new):
        return [new if k == v else r for k, r in enumerate(good)]

    def cols_scaled(v, f):
        j = good[v][2].copy()
        j[:, cols] *= f
        return swap(v, (good[v][0], good[v][1], j, good[v][3]))

    out = {FAULTS[0]: _faulty(it, oprm, good, cols_scaled(2, 0.0)), FAULTS[1]: _faulty(it, oprm, good, cols_scaled(1, 1.01))}
    out[FAULTS[2]] = _faulty(it, oprm, good, swap(1, view_rows(dec, oprm, views[1], it["views"][1], prev_code)))
    out[FAULTS[3]] = _faulty(it, oprm, good, good, n_k=good[0][2].shape[0])
    out[FAULTS[4]] = _faulty(it, oprm, good, swap(2, (good[2][0][:0], good[2][1][:0], good[2][2], good[2][3])), n_s=n_s)
    out[FAULTS[5]] = _faulty(it, oprm, good, swap(1, (good[1][0], good[1][1], good[1][2][:-3], good[1][3][:-3])), n_k=n_k)
    return out


# (seed, views) of make_object_multiview(n_surface=150, n_background=40).  The four-view seed matters for ONE fault: a 1 % error in eight
# code columns of one of FOUR views' render rows is diluted by that view's share of the pooled K and lands at TAU_H itself -- measured on
# seeds 32..36 at iterations 1 and 3: 5.4e-4 .. 4.1e-3, accepted at six of the ten states (profiles/multiview_metric.md).  Seed 32 is one
# where it clears TAU_H at both states (2.4e-3, 4.1e-3); the metric does NOT resolve that fault on every four-view object.
FAULT_OBJECTS = ((31, 3), (32, 4))
FAULT_ITERATIONS = (1, 3)


def fault_states(dec):
    """-> [(label, oprm, views, it, lin, prev_code)] at FAULT_ITERATIONS of the composed oracle's own run on FAULT_OBJECTS."""
    oprm = O.GNParams(num_iterations=1, **HYPER)
    out = []
    for seed, nv in FAULT_OBJECTS:
        obj = _mv(seed, n_views=nv, n_surface=150, n_background=40)
        tr = []
        MV.reconstruct_object_multiview(dec, oprm, obj["t"], obj["views"], trace=tr, num_iterations=max(FAULT_ITERATIONS) + 1)
        for e in FAULT_ITERATIONS:
            it, _, lin = linearise_at(dec, oprm, obj["views"], tr[e]["t_obj_cam"], tr[e]["code"])
            out.append(("%d views (seed %d), iteration %d" % (nv, seed, e), oprm, obj["views"], it, lin, tr[e - 1]["code"]))
    return out
