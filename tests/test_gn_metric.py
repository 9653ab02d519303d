"""The fp64 linearisation (oracle.dsp_oracle.linearise_fp64) and the scaled entry-by-entry metric (tests/gn_metric.py) on the CPU.

  * sanity: at the first and last recorded iteration of the small-size golden_recon_* runs, the fp64 system on the fp32 oracle's sets has
    the oracle's V and K and its loss, and its parts add up to it; the fp32 oracle's and the reference's recorded systems pass the metric
    at TAU; fp64 against itself gives zero;
  * power: faults a kernel could make -- built where possible at the level of the rows, columns and weights of J -- injected into a copy
    of the fp32 oracle's system; the unperturbed system is accepted and the faults are rejected.  What the old max-norm comparison said
    about each fault is printed, not asserted.
"""
import json
import os

import numpy as np
import pytest

import forensics as F
import gn_metric as M
from conftest import golden
from oracle import dsp_oracle as O
from dsp_slam_amd import fixtures

F32 = np.float32


def _decoder(cfg):
    name = os.path.basename(cfg.get("DeepSDF_DIR", "cars"))
    fix = "complex" if name.startswith("complex") else ("chairs32" if cfg["optimizer"]["code_len"] == 32 else "cars")
    return O.fold_decoder(fixtures.load_decoder_npz(fixtures.fixture_path(fix)), fixtures.fixture_specs(fix))


_CACHE = {}


def _state(name, e):
    """(prm, decoder, inputs, state, reference system, fp32 oracle trace, fp64 linearisation) at iteration e of a golden (memoised)."""
    key = (name, e)
    if key not in _CACHE:
        g = golden(name)
        cfg = json.loads(str(g["cfg_json"]))
        prm = O.GNParams.from_configs(cfg)
        dec = _decoder(cfg)
        e = e % g["it_H"].shape[0]
        inputs = (g["in_pts"], g["in_rays"], g["in_depth"])
        state = (g["it_t_obj_cam"][e], g["it_code"][e], g["it_depths"][e])
        it = F.oracle_linearisation(dec, prm, *inputs, *state)
        lin = O.linearise_fp64(dec, prm, *inputs, *state, it["sets"])
        ref = dict(H=g["it_H"][e], b=g["it_b"][e], dx=g["it_dx"][e], V=int(g["it_V"][e]), K=int(g["it_K"][e]))
        _CACHE[key] = (prm, dec, inputs, state, ref, it, lin)
    return _CACHE[key]


def old_max_norm_passes(sys_, it):
    """The max-norm comparison of tests/test_gpu_parity.py::compare_linearisation (without its jitter term): |dH| < 1e-4 max|H|,
    |db| < 1e-4 max|b| outside the rotation-prior entries 3:6."""
    mask = np.ones(it["b"].shape[0], bool)
    mask[3:6] = False
    h_ok = np.abs(np.asarray(sys_["H"], np.float64) - it["H"]).max() < 1e-4 * np.abs(it["H"]).max()
    b_ok = np.abs(np.asarray(sys_["b"], np.float64) - it["b"])[mask].max() < 1e-4 * np.abs(it["b"]).max()
    return bool(h_ok and b_ok)


# the cfg2-size goldens (cfg2, cfg5, complex) are too slow for the CPU tier here; their recorded states are in the measurement of
# tools/measure_gn_metric.py that fixed TAU (tests/gn_metric.py)
SANITY = ["golden_recon_%s.npz" % n for n in ("small", "cfg1", "redwood", "freiburg", "chairs32", "mono_shape", "mono_wide")]


@pytest.mark.parametrize("name", SANITY)
@pytest.mark.parametrize("which", [0, -1])
def test_fp64_linearisation_sanity(name, which):
    prm, dec, inputs, state, ref, it, lin = _state(name, which)
    # the oracle linearises on the reference's sets at its own state (test_oracle_golden); the fp64 system is on the oracle's
    assert (lin["V"], lin["K"]) == (it["V"], it["K"]) == (ref["V"], ref["K"])
    assert abs(lin["loss"] - it["loss"]) <= 1e-5 * abs(lin["loss"])
    assert lin["Lr"] > 0 and lin["Ls"] > 0 and np.all(np.diag(lin["Dr"] + lin["Ds"]) > 0)
    # the parts add up to H and b; dx solves the system
    assert np.array_equal(lin["Dr"] + lin["Ds"] + lin["H_code_prior"] + lin["H_rot"] + lin["H_damp"], lin["H"])
    assert np.array_equal(lin["gr"] + lin["gs"] + lin["b_code_prior"] + lin["b_rot"], lin["b"])
    assert np.allclose(lin["H"] @ lin["dx"], lin["b"], rtol=0, atol=1e-9 * np.abs(lin["b"]).max())
    z = M.scaled_errors(dict(H=lin["H"], b=lin["b"], dx=lin["dx"]), lin, prm.k4)
    assert max(z["worst"], z["solve"]) < 1e-12
    ro = M.scaled_errors(it, lin, prm.k4)
    rr = M.scaled_errors(ref, lin, prm.k4)
    print("%s it %d: oracle %s\n   reference %s" % (name, which, M.flat(ro), M.flat(rr)))
    M.assert_within_tau(ro, "fp32 oracle")
    M.assert_within_tau(rr, "reference")


def test_fp32_oracle_on_its_own_trajectory_is_within_tau(oracle_decoder):
    """Every iteration of the fp32 oracle's own chained run on `small` -- states the reference never visited -- within TAU of fp64.
    Iteration 2 holds a surface row whose last hidden pre-activation lies 1.2e-7 from zero: fp32 and fp64 take different sides of that
    ReLU and the row's jacobian differs by 14 %.  linearise_fp64 names such rows (H_flip / b_flip, RELU_ULPS); without that allowance the
    row alone puts the pose block 1.3e-2 from fp64."""
    g = golden("golden_recon_small.npz")
    prm = O.GNParams.from_configs(json.loads(str(g["cfg_json"])))
    tr = []
    O.reconstruct_object(oracle_decoder, prm, g["in_t_cam_obj_init"], g["in_pts"], g["in_rays"], g["in_depth"], trace=tr)
    assert len(tr) == prm.num_iterations
    for e, t in enumerate(tr):
        lin = O.linearise_fp64(oracle_decoder, prm, g["in_pts"], g["in_rays"], g["in_depth"], t["t_obj_cam"], t["code"], t["depths"], t["sets"])
        rec = M.scaled_errors(t, lin, prm.k4)
        print(e, lin["n_flip"], M.flat(rec))
        M.assert_within_tau(rec, "fp32 oracle, own trajectory, iteration %d" % e)
        if e == 2:
            assert lin["n_flip"][0] >= 1
            lin["H_flip"][:] = 0
            lin["b_flip"][:] = 0
            assert not M.within_tau(M.scaled_errors(t, lin, prm.k4)), "the kink at iteration 2 is no longer what sets this state's error"


# ---------------------------------------------------------------------------------------------------------------------------------------
# power
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rows(prm, dec, inputs, state):
    """The fp32 oracle's rows at a state: (J_s, robust r_s, J_r, robust r_r), as reconstruct_object forms them."""
    pts, rays, depth = inputs
    t, code, depths = state
    z = np.asarray(code, F32)[:prm.code_len]
    d = np.asarray(depths, F32)[:prm.num_depth_samples]
    depth_obs = np.concatenate([np.asarray(depth, F32), np.full(rays.shape[0] - depth.shape[0], F32(1.1) * d[-1], F32)]).astype(F32)
    j7s, jcs, rs = O.compute_sdf_loss(dec, pts, t, z)
    rrs = O.get_robust_res(rs, prm.b2)[0]
    j7r, jcr, rr = O.compute_render_loss(dec, rays, depth_obs, t, d, z, th=prm.cut_off)
    rrr = O.get_robust_res(rr, prm.b1)[0]
    return (np.concatenate([j7s, jcs], -1).astype(np.float64), rrs.astype(np.float64),
            np.concatenate([j7r, jcr], -1).astype(np.float64), rrr.astype(np.float64))


def _with(it, dh=None, db=None, h=None, b=None):
    """A copy of the fp32 system it with dH / db added (or H / b replaced), rounded to fp32, dx re-solved in fp32 like the reference."""
    h = (np.asarray(it["H"], np.float64) if h is None else h) + (0 if dh is None else dh)
    b = (np.asarray(it["b"], np.float64) if b is None else b) + (0 if db is None else db)
    h, b = h.astype(F32), b.astype(F32)
    return dict(H=h, b=b, dx=(np.linalg.inv(h) @ b).astype(F32))


def _column_fault(j, r, k, n, cols, eps):
    """dH, db of scaling columns `cols` of the rows j (weight k / n) by 1 + eps."""
    j2 = j.copy()
    j2[:, cols] *= 1 + eps
    return k * (j2.T @ j2 - j.T @ j) / n, -k * (j2 - j).T @ r / n


def _faults(prm, dec, inputs, state, it, lin):
    js, rs, jr, rr = _rows(prm, dec, inputs, state)
    pd = 7
    cols = pd + np.arange(8, 16)                       # eight code columns: one 8-wide fragment
    out = {}
    for eps in (1e-2, 2e-3):
        out["surface rows: 8 code columns x (1 + %g)" % eps] = _with(it, *_column_fault(js, rs, prm.k2, js.shape[0], cols, eps))
        out["render rows: 8 code columns x (1 + %g)" % eps] = _with(it, *_column_fault(jr, rr, prm.k1, jr.shape[0], cols, eps))
    # one 8x8 off-diagonal tile of the code block read from its neighbour (a wrong tile index in the Gram)
    h = np.asarray(it["H"], np.float64).copy()
    a, bt = pd, pd + 16
    h[a:a + 8, bt:bt + 8] = it["H"][a:a + 8, bt + 8:bt + 16]
    h[bt:bt + 8, a:a + 8] = h[a:a + 8, bt:bt + 8].T
    out["code block: tile (0, 2) read from (0, 3)"] = _with(it, h=h)
    # one render row's de_ds doubled: a typical contributing row (90th percentile of |J_n|), not the largest
    nrm = np.linalg.norm(jr, axis=1)
    n = int(np.argsort(nrm)[int(0.9 * (len(nrm) - 1))])
    dh = prm.k1 * 3.0 * np.outer(jr[n], jr[n]) / jr.shape[0]
    db = -prm.k1 * jr[n] * rr[n] / jr.shape[0]
    out["render row %d (90th percentile of |J|): de_ds x 2" % n] = _with(it, dh, db)
    # b's entries of one 8-dim code block x 1.01
    b = np.asarray(it["b"], np.float64).copy()
    b[pd + 16:pd + 24] *= 1.01
    out["b: code block 2 x 1.01"] = dict(_with(it, b=b), H=it["H"])
    # dx from a solve whose H has its most correlated off-diagonal code pair (relative to the data Gram) perturbed by 1 %
    sh, _ = M.scales(lin)
    rel = np.abs(lin["Dr"] + lin["Ds"]) / sh
    rel[:pd, :] = 0
    rel[:, :pd] = 0
    np.fill_diagonal(rel, 0)
    i, j = np.unravel_index(np.argmax(rel), rel.shape)
    h = np.asarray(it["H"], np.float64).copy()
    h[i, j] *= 1.01
    h[j, i] *= 1.01
    out["dx: solve with H[%d,%d] x 1.01" % (i, j)] = dict(H=it["H"], b=it["b"], dx=_with(it, h=h)["dx"])
    return out


POWER = [("golden_recon_redwood.npz", 0), ("golden_recon_redwood.npz", -1), ("golden_recon_small.npz", 0), ("golden_recon_small.npz", -1),
         ("golden_recon_chairs32.npz", 0), ("golden_recon_chairs32.npz", -1)]
# faults the metric must reject at every one of these states.  The others are printed with their scaled error.  A 1 % error in the surface
# rows' code columns is rejected at small only (accepted at redwood and chairs32, where the render rows make up almost all of the code
# columns' data Gram); the 2e-3 render-column error is accepted at small iteration 0; a 1 % error of b's code entries is accepted at small's
# last iteration (the k3 prior dominates s_i); and dx from a solve with one pair of H off by 1 % is accepted at EVERY state -- neither the
# dx residual check nor the solve-residual check sees it.
MUST_REJECT = ("render rows: 8 code columns x (1 + 0.01)", "code block: tile", "de_ds x 2")


@pytest.mark.parametrize("name,which", POWER)
def test_metric_rejects_kernel_like_faults(name, which):
    prm, dec, inputs, state, ref, it, lin = _state(name, which)
    base = M.scaled_errors(it, lin, prm.k4)
    assert M.within_tau(base), M.flat(base)
    missed, rejected = [], 0
    for what, sys_ in _faults(prm, dec, inputs, state, it, lin).items():
        rec = M.scaled_errors(sys_, lin, prm.k4)
        ok = M.within_tau(rec)
        rejected += not ok
        print("%-52s new metric: worst %.2e solve %.1e (%s)   old max-norm check: %s" % (
            what, rec["worst"], rec["solve"], "ACCEPTED" if ok else "rejected", "pass" if old_max_norm_passes(sys_, it) else "fail"))
        if ok and any(m in what for m in MUST_REJECT):
            missed.append((what, M.flat(rec)))
    assert not missed, missed
    assert rejected >= 5
