"""GPU: surface projection (include/dsp_gn.h dsp_surface_points, dsp_meshes_refine, dsp_meshes_fetch_attributes).

Plumbing is held bit for bit to dsp_sdf_jacobian + the host functions of csrc/surface_math.h (themselves pinned on the CPU by
tests/test_surface_host.py); the batched, ragged, chunked and mesh forms to each other, bit for bit; the refined meshes to the fp64 oracle
evaluated at the device's own vertices (tests/surface_ref.py), with bounds derived from the decoder tolerances of tests/test_gpu_decoders.py.
Measured figures go to the session's parity record (conftest.parity_log).
"""
import os
import sys

import numpy as np
import pytest

import surface_ref as S
from conftest import ROOT, golden, parity_log
from dsp_slam_amd import engine as E, _lib as L

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
TAU_S = 5e-6            # decode tolerance of test_gpu_decoders.py (sdf against the oracle)
STEPS = 6
NAMES = ("cars", "chairs32", "complex")


def _engine(dec):
    return E.Engine(dec.layers, dec.latent_in, dec.code_len, device=0)


@pytest.fixture(scope="module")
def decoders(oracle_decoder, chairs32_decoder, complex_decoder):
    return {"cars": oracle_decoder, "chairs32": chairs32_decoder, "complex": complex_decoder}


@pytest.fixture(scope="module")
def engines(decoders):
    es = {k: _engine(d) for k, d in decoders.items()}
    yield es
    for e in es.values():
        e.close()


def case_code(name, kind, code_len):
    """kind 0: the zero code; 1: seeded uniform +-0.3."""
    if kind == 0:
        return np.zeros(code_len, F32)
    return np.random.default_rng(100 + NAMES.index(name)).uniform(-0.3, 0.3, code_len).astype(F32)


def case_var(name, code_len):
    return np.random.default_rng(200 + NAMES.index(name)).uniform(1e-4, 4e-2, code_len)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _same_results(a, b, keys=("vertices", "normals", "sdf", "grad_norm", "sigma")):
    for k in keys:
        if k in a or k in b:
            assert _bits_equal(a[k], b[k]), k


def _jacobian_rows(eng, code, pts):
    """dsp_sdf_jacobian's raw outputs as the 68-float rows the decoder kernel writes."""
    pts = L.f32(pts).reshape(-1, 3)
    n = pts.shape[0]
    sdf, grad = np.zeros(n, F32), np.zeros((n, L.GRAD_DIM), F32)
    c = L.code64(code)
    L.check(L.load().dsp_sdf_jacobian(eng._h, L.ptr(c), L.ptr(pts), n, L.ptr(sdf), L.ptr(grad)), eng._h, "dsp_sdf_jacobian")
    return S.rows68(sdf, grad)


def _host_step(p, rows, max_step):
    p = L.f32(p).reshape(-1, 3)
    sdf, g = np.ascontiguousarray(rows[:, 67]), np.ascontiguousarray(rows[:, 64:67])
    out = np.zeros_like(p)
    if p.shape[0]:
        assert L.load().dsp_debug_surface_step(p.shape[0], L.ptr(p), L.ptr(sdf), L.ptr(g), float(max_step), L.ptr(out)) == 0
    return out


def _host_attributes(rows, var):
    n = rows.shape[0]
    nrm, gn, sdf, sig = np.zeros((n, 3), F32), np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    v = np.zeros(64)
    v[:len(var)] = var
    if n:
        assert L.load().dsp_debug_surface_attributes(n, L.ptr(rows), L.ptr(v, L.c_f64p), L.ptr(nrm), L.ptr(gn), L.ptr(sdf), L.ptr(sig)) == 0
    return nrm, gn, sdf, sig


def _points(rng, n):
    return rng.uniform(-0.6, 0.6, (n, 3)).astype(F32)


# ---- 1. plumbing, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_plumbing_is_the_jacobian_and_the_host_functions_bit_for_bit(engines, name):
    eng = engines[name]
    rng = np.random.default_rng(31)
    code, var, ms = case_code(name, 1, eng.code_len), case_var(name, eng.code_len), 0.05
    for n in (0, 1, 63, 64, 65, 130):
        p = _points(rng, n)
        rows = _jacobian_rows(eng, code, p)
        r0 = eng.surface_points([code], [p], steps=0, max_step=ms, var_code=[var])[0]
        nrm, gn, sdf, sig = _host_attributes(rows, var)
        assert r0["vertices"].shape == (n, 3) and _bits_equal(r0["vertices"], p)
        assert r0["faces"].shape == (0, 3) and _bits_equal(r0["vertices_mc"], p)
        assert _bits_equal(r0["sdf"], rows[:, 67]) and _bits_equal(r0["sdf"], sdf)
        assert _bits_equal(r0["normals"], nrm) and _bits_equal(r0["grad_norm"], gn) and _bits_equal(r0["sigma"], sig)
        r1 = eng.surface_points([code], [p], steps=1, max_step=ms)[0]
        assert "sigma" not in r1 and _bits_equal(r1["vertices"], _host_step(p, rows, ms))
        q = p
        for _ in range(3):
            q = eng.surface_points([code], [q], steps=1, max_step=ms)[0]["vertices"]
        r3 = eng.surface_points([code], [p], steps=3, max_step=ms, var_code=[var])[0]
        assert _bits_equal(r3["vertices"], q)
        _same_results(r3, eng.surface_points([code], [q], steps=0, max_step=ms, var_code=[var])[0])


# ---- 2. batched, ragged, chunked and mesh forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_ragged_chunked_and_mesh_forms_are_the_same_arithmetic(engines, name):
    eng = engines[name]
    lib = L.load()
    rng = np.random.default_rng(32)
    codes = [case_code(name, 1, eng.code_len), case_code(name, 0, eng.code_len), (0.5 * case_code(name, 1, eng.code_len)).astype(F32)]
    var = np.stack([case_var(name, eng.code_len) * (k + 1) for k in range(3)])
    pts = [_points(rng, 65), _points(rng, 0), _points(rng, 130)]
    ms = 0.04
    both = eng.surface_points(codes, pts, steps=2, max_step=ms, var_code=var)
    for i in range(3):
        _same_results(both[i], eng.surface_points([codes[i]], [pts[i]], steps=2, max_step=ms, var_code=[var[i]])[0])
    assert both[1]["vertices"].shape == (0, 3)
    # a chunk budget of 100 rows: chunks end inside objects 0 and 2
    assert lib.dsp_debug_surface_chunk_rows(eng._h, 100) == 0
    try:
        chunked = eng.surface_points(codes, pts, steps=2, max_step=ms, var_code=var)
    finally:
        assert lib.dsp_debug_surface_chunk_rows(eng._h, 0) == 0
    for a, b in zip(chunked, both):
        _same_results(a, b)
    # the mesh form: refine + fetch == dsp_surface_points on the fetched marching-cubes vertices with one voxel as the cap
    n = 16
    plain = eng.extract_meshes(codes, n)
    ref = eng.extract_meshes_refined(codes, n, steps=STEPS, var_code=var)
    nv = np.array([m["vertices_mc"].shape[0] for m in ref], np.int64)
    nf = np.array([m["faces"].shape[0] for m in ref], np.int64)
    verts, faces = np.zeros((int(nv.sum()), 3), F32), np.zeros((int(nf.sum()), 3), np.int32)
    L.check(lib.dsp_meshes_fetch(eng._h, 3, L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p), L.ptr(verts), L.ptr(faces, L.c_i32p)), eng._h, "dsp_meshes_fetch")
    assert np.array_equal(verts, np.concatenate([v for v, _ in plain])) and np.array_equal(faces, np.concatenate([f for _, f in plain]))
    direct = eng.surface_points(codes, [m["vertices_mc"] for m in ref], steps=STEPS, max_step=float(F32(2.0 / (n - 1))), var_code=var)
    for (v, f), m, d in zip(plain, ref, direct):
        assert np.array_equal(m["vertices_mc"], v) and np.array_equal(m["faces"], f) and v.shape[0] > 100
        _same_results(m, d, keys=("vertices", "normals", "sdf", "sigma"))
    assert lib.dsp_debug_surface_chunk_rows(eng._h, 100) == 0
    try:
        ref_c = eng.extract_meshes_refined(codes, n, steps=STEPS, var_code=var)
    finally:
        assert lib.dsp_debug_surface_chunk_rows(eng._h, 0) == 0
    for a, b in zip(ref_c, ref):
        _same_results(a, b, keys=("vertices", "normals", "sdf", "sigma", "vertices_mc"))


# ---- 3 - 6. refined meshes against the fp64 oracle ----------------------------------------------------------------------------------------
_CASES = {}


def refined_case(engines, decoders, name, kind, n, regular):
    """One refined mesh and the oracle at its vertices, computed once and shared by the tests below (never modified)."""
    key = (name, kind, n, regular)
    if key not in _CASES:
        eng, dec = engines[name], decoders[name]
        code, var = case_code(name, kind, eng.code_len), case_var(name, eng.code_len)
        m = eng.extract_meshes_refined([code], n, steps=STEPS, regular_grid=regular, var_code=[var])[0]
        _CASES[key] = evaluate_case(dec, code, var, m, 2.0 / (n - 1))
    return _CASES[key]


def evaluate_case(dec, code, var, m, voxel):
    """The oracle in float64 at the returned vertices, the float64 restatement's own residual from the same start, and the unrefined
    vertices' |sdf| -- everything tests 3 to 6 compare."""
    v = m["vertices"].astype(np.float64)
    y, g, g2 = S.decode64(dec, code, v)
    _, r64 = S.refine64(dec, code, m["vertices_mc"], STEPS, float(F32(voxel)))
    y_mc, _, _ = S.decode64(dec, code, m["vertices_mc"], grad=False)
    out = dict(m)
    out.update(y64=y, g64=g, g64_flip=g2, r64=float(r64.max()), sdf64_mc=np.abs(y_mc), var=var)
    return out


def check_normals(c):
    """|n_dev - n_64| <= 2 sqrt(3) tau_g / |g_xyz|, tau_g = 1e-5 max(1, max |g|) the gradient tolerance of test_gpu_decoders.py: an entry of
    the gradient is within tau_g, so |delta g|_2 <= sqrt(3) tau_g, and |delta (g / |g|)| <= 2 |delta g| / |g|.  Either side of a ReLU kink
    counts; at most 0.1 % of a case's vertices may miss, and those stay within 2e-2 / |g_xyz|."""
    tau_g = 1e-5 * max(1.0, np.abs(c["g64"]).max())
    d = []
    for g in (c["g64"], c["g64_flip"]):
        n64, gn, _, _ = S.attributes64(g, c["y64"])
        d.append(np.sqrt(((c["normals"] - n64) ** 2).sum(1)) * gn)
    d = np.minimum(d[0], d[1])
    miss = d > 2 * np.sqrt(3) * tau_g
    unit = np.abs(np.sqrt((c["normals"].astype(np.float64) ** 2).sum(1)) - 1.0).max()
    return dict(worst=float(d.max()), bound=float(2 * np.sqrt(3) * tau_g), missed=float(miss.mean()), unit=float(unit)), \
        miss.mean() <= 1e-3 and d.max() <= 2e-2 and unit <= 4 * U


def check_positions(c):
    """|sdf_64| at the device's vertices <= r64 + 2 tau_s; the unrefined vertices violate it by a factor of 100 at least."""
    bound = c["r64"] + 2 * TAU_S
    worst = float(np.abs(c["y64"]).max())
    return dict(worst=worst, bound=bound, r64=c["r64"], unrefined=float(c["sdf64_mc"].max()), dev_sdf=float(np.abs(c["sdf"]).max())), \
        worst <= bound and c["sdf64_mc"].max() > 100 * bound and np.abs(c["sdf"] - c["y64"]).max() <= TAU_S


def check_sigma(c):
    """sigma = A / B, A = sqrt(sum gc^2 var), B = |g_xyz|.  With every gradient entry within tau_g: |delta A| <= tau_g sqrt(sum var) (triangle
    inequality of the var-weighted 2-norm), |delta B| <= sqrt(3) tau_g, so |delta sigma| <= tau_g (sqrt(sum var) + sqrt(3) sigma) / B; the fp32
    arithmetic of the header adds at most 64 U sigma (tests/test_surface_host.py).  Either side of a kink; 0.1 % may miss, as for the normals."""
    tau_g = 1e-5 * max(1.0, np.abs(c["g64"]).max())
    ok, worst = None, None
    for g in (c["g64"], c["g64_flip"]):
        _, gn, _, s64 = S.attributes64(g, c["y64"], c["var"])
        bound = tau_g * (np.sqrt(c["var"].sum()) + np.sqrt(3) * s64) / gn + 64 * U * s64
        r = np.abs(c["sigma"] - s64) / bound
        ok, worst = (r <= 1, r) if ok is None else (ok | (r <= 1), np.minimum(worst, r))
    return dict(worst_ratio=float(worst.max()), missed=float(1 - ok.mean()), sigma_max=float(c["sigma"].max())), \
        (1 - ok.mean()) <= 1e-3 and np.all(c["sigma"] > 0) and np.isfinite(c["sigma"]).all()


def face_normal_dots(c):
    """dot(analytic normal, area-weighted normal of the vertex's faces), the latter normalised."""
    v, f = c["vertices"].astype(np.float64), c["faces"]
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])          # length = 2 x area
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], fn)
    acc /= np.maximum(np.sqrt((acc * acc).sum(1)), 1e-300)[:, None]
    return (acc * c["normals"]).sum(1)


GRID_CASES = [(name, kind, n, regular) for name in NAMES for kind in (0, 1) for n in (16, 32) for regular in (False, True)]


@pytest.mark.parametrize("name,kind,n,regular", GRID_CASES)
def test_refined_mesh_against_fp64(engines, decoders, name, kind, n, regular):
    c = refined_case(engines, decoders, name, kind, n, regular)
    nv = c["vertices"].shape[0]
    assert nv > 100 and c["faces"].shape[0] > 100 and np.isfinite(c["vertices"]).all()
    rn, ok_n = check_normals(c)
    rp, ok_p = check_positions(c)
    rs, ok_s = check_sigma(c)
    print(name, kind, n, regular, nv, rn, rp, rs)
    parity_log(kind="surface_refine", case="%s code %d %d^3 %s" % (name, kind, n, "regular" if regular else "sheared"), n_vertices=nv,
               normals=rn, positions=rp, sigma=rs)
    assert ok_n, rn
    assert ok_p, rp
    assert ok_s, rs
    if name != "complex":           # thin parts of `complex` fail this in fp64 too (1-3 % of the 16^3 vertices)
        dots = face_normal_dots(c)
        assert dots.min() > 0, float(dots.min())


def test_zero_variance_gives_zero_sigma_and_sigma_needs_a_variance(engines):
    eng = engines["cars"]
    lib = L.load()
    code = case_code("cars", 1, 64)
    m = eng.extract_meshes_refined([code], 16, var_code=[np.zeros(64)])[0]
    assert m["sigma"].shape[0] > 100 and np.all(m["sigma"] == 0)
    m2 = eng.extract_meshes_refined([code], 16)[0]
    assert "sigma" not in m2 and _bits_equal(m2["vertices"], m["vertices"]) and _bits_equal(m2["normals"], m["normals"])
    nv = np.array([m2["vertices"].shape[0]], np.int64)
    sig = np.zeros(int(nv[0]), F32)
    assert lib.dsp_meshes_fetch_attributes(eng._h, 1, L.ptr(nv, L.c_i64p), None, None, None, L.ptr(sig)) == -4          # DSP_E_STATE
    p = _points(np.random.default_rng(1), 5)
    off = np.array([0, 5], np.int64)
    c64 = L.code64(code)
    assert lib.dsp_surface_points(eng._h, L.ptr(c64), 1, L.ptr(off, L.c_i64p), L.ptr(p), 1, 0.1, None, None, None, None, None, L.ptr(sig)) == -1


# ---- 7. robustness -----------------------------------------------------------------------------------------------------------------------
def test_a_nan_point_disturbs_no_other_point(engines):
    eng = engines["cars"]
    code, var = case_code("cars", 1, 64), case_var("cars", 64)
    p = _points(np.random.default_rng(71), 130)
    good = eng.surface_points([code], [p], steps=3, max_step=0.05, var_code=[var])[0]
    for bad in (np.nan, np.inf):
        q = p.copy()
        q[70, 1] = bad
        r = eng.surface_points([code], [q], steps=3, max_step=0.05, var_code=[var])[0]
        keep = np.arange(130) != 70
        for k in ("vertices", "normals", "sdf", "grad_norm", "sigma"):
            assert _bits_equal(r[k][keep], good[k][keep]), k
            assert not np.isfinite(r[k][70]).all(), k
        assert np.isnan(r["sdf"][70]) and np.isnan(r["normals"][70]).any()


def test_refusals_and_state(engines, decoders):
    eng = engines["cars"]
    lib = L.load()
    codes = [case_code("cars", 1, 64), np.full(64, 3.0, F32), case_code("cars", 0, 64)]
    empty = [c for c in (np.full(64, 3.0, F32), np.full(64, -3.0, F32)) if len(eng.extract_mesh(c, 16)[1]) == 0]
    assert empty, "no code without a surface in the grid"
    codes[1] = empty[0]
    alone = eng.extract_meshes_refined([codes[2]], 16)[0]
    ms = eng.extract_meshes_refined(codes, 16)             # the handle's last extraction from here on
    assert ms[1]["vertices"].shape == (0, 3) and ms[1]["normals"].shape == (0, 3) and ms[0]["vertices"].shape[0] > 100
    _same_results(ms[2], alone, keys=("vertices", "normals", "sdf"))
    # bad arguments
    c64 = np.stack([L.code64(c) for c in codes])
    p = _points(np.random.default_rng(72), 6)
    out = np.zeros((6, 3), F32)

    def sp(off, steps=2, max_step=0.1, var=None, pts=p, n_codes=3):
        off = np.asarray(off, np.int64)
        return lib.dsp_surface_points(eng._h, L.ptr(c64), n_codes, L.ptr(off, L.c_i64p), L.ptr(pts), steps, max_step,
                                      L.ptr(var, L.c_f64p), L.ptr(out), None, None, None, None)

    assert sp([0, 2, 2, 6]) == 0
    assert sp([0, 0, 0, 0]) == 0 and sp([0, 0, 0, 0], pts=None) == 0          # a total of zero points
    for off in ([1, 2, 2, 6], [0, 3, 2, 6], [0, 2, 6, 5]):
        assert sp(off) == -1, off
    for steps in (-1, 9):
        assert sp([0, 2, 2, 6], steps=steps) == -1
    for ms_ in (0.0, -0.1, float("nan"), float("inf")):
        assert sp([0, 2, 2, 6], max_step=ms_) == -1
    assert sp([0, 2, 2, 6], pts=None) == -1 and sp([0, 2, 2, 6], n_codes=0) == -1
    for bad in (-1e-12, float("nan"), float("inf")):
        var = np.full((3, 64), 1e-3)
        var[2, 5] = bad
        assert sp([0, 2, 2, 6], var=var) == -1, bad
    assert sp([0, 2, 2, 6], var=np.full((3, 64), 1e-3)) == 0
    # state: the counts of another extraction, no refine since the last extraction
    nv = np.array([m["vertices"].shape[0] for m in ms], np.int64)
    assert lib.dsp_meshes_refine(eng._h, 3, L.ptr(nv, L.c_i64p), 9, 0.0, None) == -1
    assert lib.dsp_meshes_refine(eng._h, 3, L.ptr(nv, L.c_i64p), 2, float("nan"), None) == -1
    assert lib.dsp_meshes_refine(eng._h, 3, L.ptr(nv, L.c_i64p), 2, 0.0, None) == 0
    assert lib.dsp_meshes_refine(eng._h, 2, L.ptr(nv, L.c_i64p), 2, 0.0, None) == -4
    eng.extract_meshes(codes[:1], 20)
    assert lib.dsp_meshes_refine(eng._h, 3, L.ptr(nv, L.c_i64p), 2, 0.0, None) == -4             # a refine after another extraction
    nv1 = nv[:1].copy()
    assert lib.dsp_meshes_fetch_attributes(eng._h, 1, L.ptr(nv1, L.c_i64p), L.ptr(out), None, None, None) == -4      # no refine since
    eng2 = _engine(decoders["cars"])
    try:
        nv0 = np.array([5], np.int64)
        assert lib.dsp_meshes_refine(eng2._h, 1, L.ptr(nv0, L.c_i64p), 2, 0.0, None) == -4       # no batched extraction on the handle
    finally:
        eng2.close()


def test_allocation_failure_leaves_the_handle_and_the_meshes_usable(decoders):
    eng = _engine(decoders["chairs32"])          # a handle of its own: what it already holds decides which allocations are fresh
    try:
        _allocation_failure(eng)
    finally:
        eng.close()


def _allocation_failure(eng):
    lib = L.load()
    codes = [case_code("chairs32", 1, 32), case_code("chairs32", 0, 32)]
    plain = eng.extract_meshes(codes, 16)
    nv = np.array([v.shape[0] for v, _ in plain], np.int64)
    nf = np.array([f.shape[0] for _, f in plain], np.int64)
    p = _points(np.random.default_rng(73), 65)
    good = eng.surface_points(codes[:1], [p], steps=2, max_step=0.05)[0]
    for nth in (0, 2):
        eng.trim()                          # an empty cache: the call has to allocate afresh
        eng.fail_alloc(nth)
        with pytest.raises(L.DspError, match="out of device memory"):
            eng.surface_points(codes[:1], [p], steps=2, max_step=0.05)
        eng.fail_alloc(-1)
        eng.trim()
        _same_results(eng.surface_points(codes[:1], [p], steps=2, max_step=0.05)[0], good)
    eng.trim()
    eng.fail_alloc(0)
    assert lib.dsp_meshes_refine(eng._h, 2, L.ptr(nv, L.c_i64p), 2, 0.0, None) == -3             # DSP_E_NOMEM
    eng.fail_alloc(-1)
    eng.trim()
    verts, faces = np.zeros((int(nv.sum()), 3), F32), np.zeros((int(nf.sum()), 3), np.int32)
    L.check(lib.dsp_meshes_fetch(eng._h, 2, L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p), L.ptr(verts), L.ptr(faces, L.c_i32p)), eng._h, "dsp_meshes_fetch")
    assert np.array_equal(verts, np.concatenate([v for v, _ in plain])) and np.array_equal(faces, np.concatenate([f for _, f in plain]))
    assert lib.dsp_meshes_refine(eng._h, 2, L.ptr(nv, L.c_i64p), 2, 0.0, None) == 0


# ---- 8. mirror and tool ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def mirror():
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    sys.path.insert(0, pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    yield
    sys.path.remove(pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]


def test_mirror_and_remesh_tool(tmp_path, mirror, oracle_decoder):
    import test_gpu_map_tools as T
    from dsp_slam_amd.map_objects import read_map_objects, write_map_objects
    from reconstruct.utils import get_configs, get_decoder, write_mesh_to_ply, read_mesh_from_ply_with_normals
    from reconstruct.optimizer import MeshExtractor
    g = golden("golden_map_objects.npz")
    dirs = []
    for tag in ("plain", "refined"):
        d = tmp_path / tag
        d.mkdir()
        with open(d / "MapObjects.txt", "wb") as f:
            f.write(g["text"].tobytes())
        objs = read_map_objects(str(d / "MapObjects.txt"))
        for o, c3 in zip(objs[:2], ((0.3, -0.2, 0.1), (-0.4, 0.5, 0.0))):       # two objects with a real shape, as test_gpu_map_tools.py
            o["code"] = np.zeros(64, F32)
            o["code"][:3] = c3
        write_map_objects(str(d / "MapObjects.txt"), objs)
        dirs.append(d)
    objs = read_map_objects(str(dirs[0] / "MapObjects.txt"))
    cfg_path = T._config(tmp_path)
    n = 16
    T._run_tool("remesh_map.py", ["--config", cfg_path, "--map_dir", str(dirs[0]), "--voxels_dim", str(n)])
    T._run_tool("remesh_map.py", ["--config", cfg_path, "--map_dir", str(dirs[1]), "--voxels_dim", str(n), "--refine", str(STEPS)])
    cfg = get_configs(cfg_path)
    ext = MeshExtractor(get_decoder(cfg), cfg.optimizer.code_len, n)
    codes = [o["code"] for o in objs]
    mirror_meshes = ext.extract_refined_meshes_from_codes(codes, steps=STEPS)
    engine_meshes = ext.decoder.engine.extract_meshes_refined([np.asarray(c, F32)[:64] for c in codes], n, steps=STEPS)
    n_mesh = 0
    for o, mm, em in zip(objs, mirror_meshes, engine_meshes):
        _same_results(mm, em, keys=("vertices", "normals", "sdf", "vertices_mc"))
        assert np.array_equal(mm.faces, em["faces"])
        ply = dirs[1] / "objects" / ("%d.ply" % o["id"])
        plain = dirs[0] / "objects" / ("%d.ply" % o["id"])
        assert ply.exists() == plain.exists() == (mm.vertices.shape[0] > 0)
        if not ply.exists():
            continue
        # without --refine: the file of today, byte for byte -- the marching-cubes mesh in the plain layout
        write_mesh_to_ply(mm.vertices_mc, mm.faces, str(tmp_path / "expect.ply"))
        assert open(str(plain), "rb").read() == open(str(tmp_path / "expect.ply"), "rb").read()
        v, nrm, f, q = read_mesh_from_ply_with_normals(str(ply))
        assert q is None and _bits_equal(v, mm.vertices) and _bits_equal(nrm, mm.normals) and np.array_equal(f, mm.faces)
        assert np.abs(np.sqrt((nrm.astype(np.float64) ** 2).sum(1)) - 1.0).max() <= 4 * U
        c = evaluate_case(oracle_decoder, np.asarray(o["code"], F32)[:64], np.zeros(64), dict(mm), 2.0 / (n - 1))
        rp, ok = check_positions(c)
        assert ok, rp
        n_mesh += 1
    assert n_mesh >= 2
