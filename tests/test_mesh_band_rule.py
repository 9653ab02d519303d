"""CPU: the surface-band selection rule of batched mesh extraction (dsp_extract_meshes, k_mesh_band in mesh_kernels.hip), stated in
numpy and checked against the marching-cubes oracle.

A prepass value lp is certain `+` when lp >= delta, certain `-` when lp <= -delta, uncertain otherwise (NaN and inf included).  A grid
point gets its fp32 value when it is uncertain or when one of its <= 6 axis neighbours is uncertain or certain of the other sign.  Claim:
if |lp - fp32| < delta everywhere, then every unselected entry may hold ANY value of its certified sign within delta of the fp32 value
and marching cubes still returns exactly the fp32 volume's mesh.  Checked on fixture-decoder grids (oracle decode) and on noise volumes
with exact zeros, NaNs and +-delta ties; and the neighbour clause is shown to be needed.
"""
import numpy as np
import pytest

from oracle import dsp_oracle as O, mc_oracle as M
from dsp_slam_amd import fixtures


def classify(lp, delta):
    fin = np.isfinite(lp)
    with np.errstate(invalid="ignore"):
        return np.where(fin & (lp >= delta), 1, np.where(fin & (lp <= -delta), -1, 0)).astype(np.int8)


def select(lp, delta, neighbours=True):
    cls = classify(lp, delta)
    need = cls == 0
    if neighbours:
        for ax in range(3):
            for sh in (1, -1):
                nb = np.roll(cls, sh, axis=ax)
                ok = np.ones(cls.shape, bool)        # neighbour inside the grid (no wrap-around)
                idx = [slice(None)] * 3
                idx[ax] = 0 if sh == 1 else -1
                ok[tuple(idx)] = False
                need |= ok & (nb != cls)
    return need, cls


def band_volume(fp32, lp, delta, rng, neighbours=True, extreme=False):
    """What the device holds before marching cubes: fp32 where selected, elsewhere an arbitrary value of the certified sign within
    delta of the fp32 value (extreme: as far from it as allowed)."""
    need, cls = select(lp, delta, neighbours)
    r = np.sign(rng.uniform(-1, 1, fp32.shape)) if extreme else rng.uniform(-1, 1, fp32.shape)
    with np.errstate(invalid="ignore"):
        other = (fp32 + r * np.float32(0.999 * delta)).astype(np.float32)
        # keep the certified sign (an fp32 value of that class is >= delta away from 0 minus the lp error, so this is within delta)
        other = np.where(cls > 0, np.maximum(other, np.float32(delta * 1e-3)), np.where(cls < 0, np.minimum(other, np.float32(-delta * 1e-3)), other))
    return np.where(need, fp32, other).astype(np.float32)


def same_mesh(a, b):
    va, fa = M.marching_cubes(a)
    vb, fb = M.marching_cubes(b)
    return va.shape == vb.shape and fa.shape == fb.shape and np.array_equal(va, vb, equal_nan=True) and np.array_equal(fa, fb)


def _decoder_grids():
    out = []
    for name, codes in (("cars", [(0.3, -0.2, 0.1), (0.2, -0.3, 0.15)]), ("chairs32", [(0.25, -0.1, 0.05)]), ("complex", [None])):
        dec = O.fold_decoder(fixtures.load_decoder_npz(fixtures.fixture_path(name)), fixtures.fixture_specs(name))
        rng = np.random.default_rng(len(name))
        for c3 in codes:
            code = (rng.normal(0, 0.1, dec.code_len) if c3 is None else np.r_[c3, rng.normal(0, 0.01, dec.code_len - 3)]).astype(np.float32)
            for n in (16, 32):
                g = np.linspace(-1, 1, n, dtype=np.float32)
                pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
                out.append(("%s %d" % (name, n), O.decode_sdf(dec, code, pts).astype(np.float32).reshape(n, n, n)))
    return out


def _noise_volumes(delta):
    rng = np.random.default_rng(5)
    out = []
    for k, shape in enumerate([(9, 11, 7), (16, 16, 16), (20, 6, 13)]):
        v = (rng.normal(size=shape) * 4 * delta).astype(np.float32)
        u = rng.random(shape)
        v[u < 0.05] = 0.0
        v[(u >= 0.05) & (u < 0.1)] = np.float32(delta)
        v[(u >= 0.1) & (u < 0.15)] = np.float32(-delta)
        if k == 1:
            v[u > 0.98] = np.nan
        out.append(("noise %d" % k, v))
    return out


_GRIDS = None


def grids():
    global _GRIDS
    if _GRIDS is None:
        _GRIDS = _decoder_grids()
    return _GRIDS


@pytest.mark.parametrize("delta", [1e-3, 4e-3])
def test_band_rule_is_exact(delta):
    rng = np.random.default_rng(int(delta * 1e4))
    for name, fp32 in grids() + _noise_volumes(delta):
        for extreme in (False, True):
            # the issue's statement: the fp32 value stands in for the prepass value
            assert same_mesh(band_volume(fp32, fp32, delta, rng, extreme=extreme), fp32), name
            # a prepass value off by up to delta / 2 (the guard's trip point): selection on it, unselected entries keep it
            with np.errstate(invalid="ignore"):
                lp = (fp32 + rng.uniform(-0.499, 0.499, fp32.shape) * delta).astype(np.float32)
            need, _ = select(lp, delta)
            assert same_mesh(np.where(need, fp32, lp).astype(np.float32), fp32), name


def test_band_fraction_of_the_decoder_grids():
    for name, fp32 in grids():
        need, _ = select(fp32, 1e-3)
        frac = need.mean()
        assert 0.0 < frac < (0.3 if name.endswith(" 16") else 0.15), (name, frac)


def test_neighbour_clause_is_needed():
    delta = 1e-3
    rng = np.random.default_rng(0)
    failures = 0
    for name, fp32 in grids() + _noise_volumes(delta):
        if not same_mesh(band_volume(fp32, fp32, delta, rng, neighbours=False, extreme=True), fp32):
            failures += 1
    assert failures >= 1
