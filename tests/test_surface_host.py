"""CPU-only: surface projection (dsp_surface_points / dsp_meshes_refine, include/dsp_gn.h) above and below the device.

  * every new symbol is declared in the header, exported by the library and bound in dsp_slam_amd/_lib.py;
  * the arithmetic: dsp_debug_surface_step / dsp_debug_surface_attributes (csrc/surface_math.h, the functions the device kernels call)
    against the numpy float32 restatement of the same single operations in the same order (tests/surface_ref.py), bit for bit, on random
    rows and on the edge cases: a zero gradient, a gradient below TINY, a step exactly at the cap, NaN and inf -- the fixed summation
    tree included;
  * the same functions against float64 on the same inputs, with derived bounds;
  * every refusal that needs no device;
  * the PLY with normals round trip; the plain PLY reader and writer are unchanged.
"""
import os
import re
import sys

import numpy as np
import pytest

import surface_ref as S
from conftest import ROOT
from dsp_slam_amd import _lib as L

F32 = np.float32
U = 2.0 ** -24          # unit round-off of fp32
NEW = ["dsp_surface_points", "dsp_meshes_refine", "dsp_meshes_fetch_attributes", "dsp_debug_surface_step", "dsp_debug_surface_attributes",
       "dsp_debug_surface_chunk_rows"]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    """bit equality, any NaN equal to any NaN (the payload of a NaN is not part of the contract)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def host_step(p, sdf, g, max_step):
    p, sdf, g = L.f32(p).reshape(-1, 3), L.f32(sdf).reshape(-1), L.f32(g).reshape(-1, 3)
    out = np.full_like(p, 7.0)
    assert L.load().dsp_debug_surface_step(p.shape[0], L.ptr(p), L.ptr(sdf), L.ptr(g), float(max_step), L.ptr(out)) == 0
    return out


def host_attributes(rows, var=None):
    rows = L.f32(rows).reshape(-1, 68)
    n = rows.shape[0]
    nrm, gn, sdf = np.full((n, 3), 7.0, F32), np.full(n, 7.0, F32), np.full(n, 7.0, F32)
    sig = np.full(n, 7.0, F32) if var is not None else None
    v = None if var is None else np.ascontiguousarray(var, np.float64)
    assert L.load().dsp_debug_surface_attributes(n, L.ptr(rows), L.ptr(v, L.c_f64p), L.ptr(nrm), L.ptr(gn), L.ptr(sdf), L.ptr(sig)) == 0
    return nrm, gn, sdf, sig


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dsp_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    bound = {n for n, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert not [n for n in NEW if n.startswith("dsp_batch_set_")] and lib.dsp_abi_version() == 6


def _random_step_inputs(rng, n):
    p = rng.uniform(-1, 1, (n, 3)).astype(F32)
    g = (rng.normal(size=(n, 3)) * rng.uniform(0.05, 1.6, (n, 1))).astype(F32)
    sdf = (rng.normal(size=n) * 0.05).astype(F32)
    return p, sdf, g


def _edge_step_inputs(max_step):
    ms = F32(max_step)
    p = np.tile(np.array([[0.25, -0.5, 0.125]], F32), (12, 1))
    g = np.tile(np.array([[0.0, 1.0, 0.0]], F32), (12, 1))
    sdf = np.full(12, 0.01, F32)
    g[0] = 0.0                                       # zero gradient: stays
    g[1] = (5e-11, 0.0, 0.0)                         # |g|^2 = 2.5e-21 < TINY: stays
    g[2] = (2e-10, 0.0, 0.0)                         # |g|^2 = 4e-20 >= TINY: a huge Newton step, capped
    sdf[3] = ms                                      # unit gradient: |d| == max_step exactly -- not scaled
    sdf[4] = np.nextafter(ms, F32(1))                # one ulp beyond the cap
    sdf[5] = np.nan
    sdf[6] = np.inf
    g[7, 1] = np.nan
    g[8, 0] = np.inf
    p[9, 2] = np.nan                                 # a NaN point stays NaN
    p[10, 0] = np.inf
    g[11] = (3e19, 3e19, 0.0)                        # |g|^2 overflows: stays
    return p, sdf, g


@pytest.mark.parametrize("max_step", [0.0625, 0.1333333, 1e-3])
def test_step_is_the_float32_restatement_bit_for_bit(max_step):
    rng = np.random.default_rng(11)
    p, sdf, g = _random_step_inputs(rng, 4000)
    sdf[::3] *= 20.0                                 # a third of the steps beyond the cap
    pe, se, ge = _edge_step_inputs(max_step)
    p, sdf, g = np.concatenate([p, pe]), np.concatenate([sdf, se]), np.concatenate([g, ge])
    got, want = host_step(p, sdf, g, max_step), S.step32(p, sdf, g, max_step)
    assert _same_bits(got, want)
    e = got[-12:]
    for k in (0, 1, 5, 6, 7, 8, 11):                 # the point does not move
        assert _same_bits(e[k], pe[k]), k
    assert np.isnan(e[9, 2]) and _same_bits(e[9, :2], S.step32(pe[9:10], se[9:10], ge[9:10], max_step)[0, :2])
    ms = F32(max_step)
    assert e[3, 1] == F32(F32(-0.5) - ms) and e[2, 0] == F32(F32(0.25) - ms)        # at the cap unscaled / capped to exactly max_step along x
    moved = np.sqrt(((got[:4000].astype(np.float64) - p[:4000]) ** 2).sum(1))
    # (the difference p - p' carries the rounding of p' itself: U per coordinate of a point inside [-1.1, 1.1]^3)
    assert moved.max() <= max_step * (1 + 8 * U) + 1.1 * np.sqrt(3) * U and (moved > 0.99 * max_step).any() and (moved < 0.5 * max_step).any()


def _random_rows(rng, n):
    rows = (rng.normal(size=(n, 68)) * rng.uniform(1e-3, 2.0, (n, 1))).astype(F32)
    rows[:, 64:67] = (rng.normal(size=(n, 3)) * rng.uniform(0.15, 1.6, (n, 1))).astype(F32)
    rows[:, 67] = (rng.normal(size=n) * 0.05).astype(F32)
    return rows


def _edge_rows(rng):
    rows = _random_rows(rng, 6)
    rows[0, 64:67] = 0.0                             # zero gradient: zero normal, zero sigma
    rows[1, 64:67] = (5e-11, 0.0, 0.0)               # below TINY
    rows[2, 65] = np.nan
    rows[3, 64] = np.inf
    rows[4, 10] = np.nan                             # a NaN code gradient: only sigma is NaN
    rows[5, 67] = np.nan
    return rows


def test_attributes_are_the_float32_restatement_bit_for_bit():
    rng = np.random.default_rng(12)
    rows = np.concatenate([_random_rows(rng, 3000), _edge_rows(rng)])
    for var in (None, rng.uniform(0.0, 0.04, 64), np.zeros(64), 10.0 ** rng.uniform(-12, 2, 64)):
        got, want = host_attributes(rows, var), S.attributes32(rows, var)
        for k, name in enumerate(("normal", "grad_norm", "sdf")):
            assert _same_bits(got[k], want[k]), name
        if var is None:
            assert got[3] is None
        else:
            assert _same_bits(got[3], want[3])
            e = got[3][-6:]
            assert e[0] == 0 and e[1] == 0 and np.isnan(e[2]) and np.isnan(e[4]) and np.isfinite(e[5])
            if not np.any(var):
                assert np.all(got[3][:3000] == 0)
        e = got[0][-6:]
        assert np.all(e[0] == 0) and np.all(e[1] == 0) and np.isnan(e[2]).any() and np.isfinite(e[4]).all()
        assert np.isnan(got[2][-1]) and np.isfinite(got[0][-1]).all()


def test_summation_tree_is_the_one_in_the_header():
    """Terms chosen so that another order gives other bits: the tree's value differs from numpy's pairwise / sequential sums somewhere."""
    rng = np.random.default_rng(13)
    rows = _random_rows(rng, 2000)
    rows[:, 64:67] = (1.0, 0.0, 0.0)                 # |g| = 1: sigma = sqrt(S)
    var = 10.0 ** rng.uniform(-6, 0, 64)
    sig = host_attributes(rows, var)[3]
    terms = (rows[:, :64] * rows[:, :64]) * var.astype(F32)[None, :]
    assert _same_bits(sig, np.sqrt(S.tree_sum32(terms)))
    seq = np.zeros(2000, F32)
    for k in range(64):
        seq = seq + terms[:, k]
    assert (_bits(np.sqrt(seq)) != _bits(sig)).any()


def test_host_functions_against_float64():
    """On the same fp32 inputs.  sigma^2 = S / |g|^2: S is a 64-term sum of non-negative fp32 terms, each two roundings from exact, summed
    in a tree of depth 7 -- within 64 U of exact in the worst case; |g|^2 (3 U), the two square roots and the division add less than 8 U;
    the bound 2 * 64 * U covers both.  A normal's component: |g|^2 carries <= 3 U (products U, two additions of positives 2 U),
    sqrt halves it and rounds (2.5 U), the division rounds (3.5 U) -> 4 U relative to the component."""
    rng = np.random.default_rng(14)
    rows = _random_rows(rng, 5000)
    var = rng.uniform(0.0, 0.04, 64)
    nrm, gn, sdf, sig = host_attributes(rows, var)
    r64 = rows.astype(np.float64)
    n64, gn64, _, s64 = S.attributes64(np.concatenate([r64[:, :64], r64[:, 64:67]], 1), r64[:, 67], var.astype(F32).astype(np.float64))
    assert np.all(np.abs(nrm - n64) <= 4 * U * np.abs(n64) + 1e-45)
    assert np.all(np.abs(gn - gn64) <= 3 * U * gn64)
    assert np.all(np.abs(sig.astype(np.float64) ** 2 - s64 ** 2) <= 2 * 64 * U * s64 ** 2)
    p, sd, g = _random_step_inputs(rng, 5000)
    for ms in (0.0625, 1e-3):
        got = host_step(p, sd, g, ms)
        want = S.step64(p, sd, g, ms)
        # d carries <= 8 U relative (|g|^2 3 U, the quotient, the product, the cap's norm, root, quotient and product); p - d rounds once more
        d = np.abs(want - p.astype(np.float64))
        near_cap = np.abs(np.sqrt((d * d).sum(1)) - ms) <= 8 * U * ms          # either side of the cap: both are within the bound of each other
        assert np.all(np.abs(got - want) <= 8 * U * d + U * np.abs(want) + 8 * U * ms * near_cap[:, None])


def test_refusals_that_need_no_device():
    lib = L.load()
    z = np.zeros(64, F32)
    off = np.array([0, 2], np.int64)
    p = np.zeros((2, 3), F32)
    o = np.zeros((2, 3), F32)
    v = np.zeros(64, np.float64)

    def sp(h=None, codes=z, n_codes=1, off_=off, pts=p, steps=6, ms=0.1):
        return lib.dsp_surface_points(h, L.ptr(codes), n_codes, L.ptr(off_, L.c_i64p), L.ptr(pts), steps, ms, None, L.ptr(o), None, None, None, None)

    assert sp() == -1                                                   # DSP_E_ARG: no handle
    nv = np.array([2], np.int64)
    assert lib.dsp_meshes_refine(None, 1, L.ptr(nv, L.c_i64p), 6, 0.0, None) == -1
    assert lib.dsp_meshes_fetch_attributes(None, 1, L.ptr(nv, L.c_i64p), L.ptr(o), None, None, None) == -1
    assert lib.dsp_debug_surface_chunk_rows(None, 100) == -1
    s1, g = np.zeros(2, F32), np.zeros((2, 3), F32)
    assert lib.dsp_debug_surface_step(2, L.ptr(p), L.ptr(s1), L.ptr(g), 0.1, L.ptr(o)) == 0
    assert lib.dsp_debug_surface_step(0, None, None, None, 0.1, None) == 0
    for ms in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dsp_debug_surface_step(2, L.ptr(p), L.ptr(s1), L.ptr(g), ms, L.ptr(o)) == -1, ms
    assert lib.dsp_debug_surface_step(-1, L.ptr(p), L.ptr(s1), L.ptr(g), 0.1, L.ptr(o)) == -1
    assert lib.dsp_debug_surface_step(2, None, L.ptr(s1), L.ptr(g), 0.1, L.ptr(o)) == -1
    assert lib.dsp_debug_surface_step(2, L.ptr(p), L.ptr(s1), L.ptr(g), 0.1, None) == -1
    rows = np.zeros((2, 68), F32)
    assert lib.dsp_debug_surface_attributes(2, None, None, L.ptr(o), None, None, None) == -1
    assert lib.dsp_debug_surface_attributes(2, L.ptr(rows), None, None, None, None, L.ptr(s1)) == -1          # sigma without a variance
    for bad in (-1e-9, float("nan"), float("inf")):
        vb = v.copy()
        vb[17] = bad
        assert lib.dsp_debug_surface_attributes(2, L.ptr(rows), L.ptr(vb, L.c_f64p), None, None, None, L.ptr(s1)) == -1, bad
    assert lib.dsp_debug_surface_attributes(2, L.ptr(rows), L.ptr(v, L.c_f64p), None, None, None, L.ptr(s1)) == 0


@pytest.fixture()
def mirror():
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    sys.path.insert(0, pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    yield
    sys.path.remove(pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]


def test_ply_with_normals_round_trip(tmp_path, mirror):
    from reconstruct import utils as RU
    rng = np.random.default_rng(15)
    v, n = rng.normal(size=(37, 3)).astype(F32), rng.normal(size=(37, 3)).astype(F32)
    f = rng.integers(0, 37, (50, 3)).astype(np.int32)
    q = rng.uniform(0, 1, 37).astype(F32)
    for quality in (None, q):
        path = str(tmp_path / ("m%d.ply" % (quality is not None)))
        RU.write_mesh_to_ply_with_normals(v, n, f, path, quality=quality)
        v2, n2, f2, q2 = RU.read_mesh_from_ply_with_normals(path)
        assert np.array_equal(v2, v) and np.array_equal(n2, n) and np.array_equal(f2, f)
        assert (q2 is None) if quality is None else np.array_equal(q2, q)
        head = open(path, "rb").read().split(b"end_header\n")[0].decode()
        assert "property float nx" in head and ("property float quality" in head) == (quality is not None)
    with pytest.raises(ValueError):
        RU.write_mesh_to_ply_with_normals(v, n[:5], f, str(tmp_path / "bad.ply"))
    # the plain layout is what it was: 12 bytes per vertex, 13 per face, and its reader refuses nothing it read before
    plain = str(tmp_path / "plain.ply")
    RU.write_mesh_to_ply(v, f, plain)
    data = open(plain, "rb").read()
    assert len(data) == data.index(b"end_header\n") + 11 + 37 * 12 + 50 * 13 and b"nx" not in data.split(b"end_header\n")[0]
    v3, f3 = RU.read_mesh_from_ply(plain)
    assert np.array_equal(v3, v) and np.array_equal(f3, f)
    with pytest.raises(ValueError):
        RU.read_mesh_from_ply_with_normals(plain)
