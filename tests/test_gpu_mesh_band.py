"""GPU: batched mesh extraction with the surface band (include/dsp_gn.h dsp_extract_meshes, DESIGN.md "Mesh extraction").

The low-precision prepass decodes every grid point; only the points whose sign it cannot certify, their axis neighbours and a fixed
audit sample go through the fp32 kernel.  Every mesh must equal, bit for bit and in the same order, what dsp_extract_mesh returns
without a prepass -- on the three fixture decoders, both grid forms, 32^3 to 128^3, 1 to 64 objects, codes up to |z|inf = 2 -- with the
guard silent.  A forced margin of 1e-7 must trip it, re-run the tripped objects densely, keep the bits and leave the handle's prepass
margins (and so a Gauss-Newton run after it) as they were.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, golden
from dsp_slam_amd import fixtures, synth, engine as E, _lib as L

pytestmark = pytest.mark.gpu


def _engine(dec):
    return E.Engine(dec.layers, dec.latent_in, dec.code_len, device=0)


@pytest.fixture(scope="module")
def engines(oracle_decoder, chairs32_decoder, complex_decoder):
    es = {"cars": _engine(oracle_decoder), "chairs32": _engine(chairs32_decoder), "complex": _engine(complex_decoder)}
    yield es
    for e in es.values():
        e.close()


def _codes(name, n, seed, code_len):
    """Warm-start-like codes of the fixture's family; every third one scaled so that its largest entry is 1 or 2."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if name == "complex":
            c = rng.normal(0.0, 0.1, code_len)
        else:
            c = rng.normal(0.0, 0.02, code_len)
            c[:3] = rng.uniform((0.15, -0.35, -0.1), (0.4, 0.0, 0.2))
        if i % 3 == 2:
            c = c * ((1.0 + (i % 2)) / np.abs(c).max())
        out.append(c.astype(np.float32))
    return out


def _dense(eng, codes, n, regular):
    return [eng.extract_mesh(c, n, regular_grid=regular) for c in codes]


def _same(got, want):
    assert len(got) == len(want)
    for i, ((v, f), (ov, of)) in enumerate(zip(got, want)):
        assert v.shape == ov.shape and f.shape == of.shape, (i, v.shape, ov.shape, f.shape, of.shape)
        assert np.array_equal(v, ov) and np.array_equal(f, of), i


CASES = [   # decoder, vol_dim, n objects, regular grid, prepass
    ("cars", 32, 17, False, "f16"),
    ("cars", 64, 3, True, "bf16"),
    ("cars", 64, 64, False, "f16"),
    ("cars", 128, 1, False, "bf16"),
    ("chairs32", 32, 64, True, "bf16"),
    ("chairs32", 64, 17, False, "f16"),
    ("chairs32", 128, 3, True, "f16"),
    ("complex", 32, 1, False, "bf16"),
    ("complex", 64, 17, True, "f16"),
    ("complex", 128, 3, False, "bf16"),
]


@pytest.mark.parametrize("name,n,n_obj,regular,prepass", CASES)
def test_band_meshes_equal_dense_meshes(engines, name, n, n_obj, regular, prepass):
    eng = engines[name]
    codes = _codes(name, n_obj, 7 * n + n_obj, eng.code_len)
    got = eng.extract_meshes(codes, n, regular_grid=regular, prepass=prepass)
    st = eng.mesh_stats()
    _same(got, _dense(eng, codes, n, regular))
    assert st["reruns"] == 0 and st["dense_points"] == 0, st
    assert st["prepass_points"] == n_obj * n ** 3 and 0 < st["band_points"] and 0 < st["audit_points"]
    assert sum(len(f) for _, f in got) > 0


def test_single_object_prepass_flag(engines):
    eng = engines["cars"]
    for prepass in ("f16", "bf16"):
        for c in _codes("cars", 3, 11, 64):
            v, f = eng.extract_mesh(c, 48, prepass=prepass)
            assert eng.mesh_stats()["reruns"] == 0
            ov, of = eng.extract_mesh(c, 48)
            assert np.array_equal(v, ov) and np.array_equal(f, of) and len(f) > 0


def test_empty_objects_in_a_batch(engines):
    eng = engines["cars"]
    # the recorded map's codes are random (tools/make_golden_map.py): some give no surface inside the grid
    cand = [np.asarray(c, np.float32).reshape(-1)[:64] for c in golden("golden_map_objects.npz")["codes"]]
    cand += [np.full(64, 3.0, np.float32), np.full(64, -3.0, np.float32)]
    empty = [c for c in cand if len(eng.extract_mesh(c, 32)[1]) == 0]
    assert empty, "no candidate code without a surface in the grid"
    good = _codes("cars", 2, 5, 64)
    codes = [good[0], empty[0], good[1]]
    want = _dense(eng, codes, 32, False)
    for prepass in (None, "f16"):
        got = eng.extract_meshes(codes, 32, prepass=prepass)
        assert got[1][0].shape == (0, 3) and got[1][1].shape == (0, 3)
        _same(got, want)


@pytest.mark.parametrize("regular", [False, True])
def test_dense_batched_path(engines, regular):
    eng = engines["complex"]
    codes = _codes("complex", 5, 3, 64)
    got = eng.extract_meshes(codes, 40, regular_grid=regular)
    st = eng.mesh_stats()
    assert st["prepass_points"] == 0 and st["band_points"] == 0 and st["dense_points"] == 5 * 40 ** 3
    _same(got, _dense(eng, codes, 40, regular))


def test_forced_margin_trips_and_reruns(engines):
    eng = engines["cars"]
    obj = synth.make_object(77, n_surface=120, n_background=30)
    prm = E.gn_params(num_iterations=3)

    def gn():
        b = eng.batch(prm, [obj["t_cam_obj_init"]], [obj["pts"]], [obj["rays"]], [obj["depth"]])
        b.run()
        r = b.results()
        b.close()
        return r

    before = gn()
    table = eng.prepass_calibration_table(L.PREPASS_F16)
    codes = _codes("cars", 4, 21, 64)
    got = eng.extract_meshes(codes, 48, prepass="f16", delta=1e-7)
    st = eng.mesh_stats()
    _same(got, _dense(eng, codes, 48, False))
    assert st["reruns"] == 4 and st["dense_points"] == 4 * 48 ** 3 and st["max_guard_err"] > 0, st
    after_table = eng.prepass_calibration_table(L.PREPASS_F16)
    for k in ("delta", "max_err"):
        assert np.array_equal(table[k], after_table[k])
    assert table["guard_err"] == after_table["guard_err"]
    after = gn()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_band_fraction_at_64(engines):
    eng = engines["cars"]
    codes = _codes("cars", 16, 64, 64)
    eng.extract_meshes(codes, 64, prepass="f16")
    st = eng.mesh_stats()
    assert st["prepass_points"] == 16 * 64 ** 3
    frac = (st["band_points"] + st["audit_points"]) / st["prepass_points"]
    print("cars 64^3 x 16, f16: fp32 fraction %.4f (band %d, audit %d)" % (frac, st["band_points"], st["audit_points"]))
    assert frac < 0.15 and st["reruns"] == 0


def test_chunked_request(engines):
    """128^3 x 64 objects does not fit one chunk of the device budget: the chunked result is the per-object one."""
    eng = engines["cars"]
    codes = _codes("cars", 64, 128, 64)
    got = eng.extract_meshes(codes, 128, prepass="f16")
    assert eng.mesh_stats()["reruns"] == 0
    _same(got, _dense(eng, codes, 128, False))


def test_errors(engines, oracle_decoder):
    import copy
    from oracle import dsp_oracle as O
    eng = engines["cars"]
    lib = L.load()
    code = np.stack(_codes("cars", 2, 1, 64))
    nv, nf = np.zeros(2, np.int64), np.zeros(2, np.int64)
    pv, pf = L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p)

    def call(n_codes=2, vol_dim=16, flags=L.MESH_PREPASS_F16, delta=0.0):
        return lib.dsp_extract_meshes(eng._h, L.ptr(code), n_codes, vol_dim, flags, delta, pv, pf)

    assert call(n_codes=0) == -1 and call(vol_dim=1) == -1 and call(vol_dim=513) == -1
    assert call(flags=L.MESH_PREPASS_F16 | L.MESH_PREPASS_BF16) == -1 and call(flags=8) == -1 and call(delta=float("nan")) == -1
    nv1, nf1 = C.c_int64(0), C.c_int64(0)
    assert lib.dsp_extract_mesh(eng._h, L.ptr(code), 16, L.MESH_PREPASS_F16 | L.MESH_PREPASS_BF16, C.byref(nv1), C.byref(nf1)) == -1
    assert call() == 0
    verts = np.zeros((int(nv.sum()), 3), np.float32)
    faces = np.zeros((int(nf.sum()), 3), np.int32)
    fv, ff = L.ptr(verts), L.ptr(faces, L.c_i32p)
    assert lib.dsp_meshes_fetch(eng._h, 1, pv, pf, fv, ff) == -4
    bad = nv.copy()
    bad[1] += 1
    assert lib.dsp_meshes_fetch(eng._h, 2, L.ptr(bad, L.c_i64p), pf, fv, ff) == -4
    assert lib.dsp_meshes_fetch(eng._h, 2, pv, pf, fv, ff) == 0
    # a decoder the prepass kernel does not take (7 hidden layers): the flags are refused, the dense batched path works
    sp = copy.deepcopy(fixtures.SPECS)
    sp["NetworkSpecs"].update(dims=[512] * 7, latent_in=[4], norm_layers=list(range(7)), dropout=list(range(7)))
    dec = O.fold_decoder(fixtures.random_state_dict(12, sp), sp)
    e7 = _engine(dec)
    try:
        rc = lib.dsp_extract_meshes(e7._h, L.ptr(code), 2, 16, L.MESH_PREPASS_F16, 0.0, pv, pf)
        assert rc == -1 and b"prepass" in lib.dsp_last_error(e7._h)
        with pytest.raises(L.DspError):
            e7.extract_mesh(code[0], 16, prepass="bf16")
        codes7 = [code[0] * 3.0, code[1]]
        _same(e7.extract_meshes(codes7, 24), _dense(e7, codes7, 24, False))
    finally:
        e7.close()


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


def test_mesh_extractor_batched_mirror(cars_state_dict, mirror):
    from reconstruct.optimizer import MeshExtractor
    from deep_sdf.workspace import decoder_from_state_dict
    dec = decoder_from_state_dict(cars_state_dict, fixtures.SPECS, device=0)
    codes = _codes("cars", 6, 99, 64)
    got = MeshExtractor(dec, 64, 64, prepass="f16").extract_meshes_from_codes(codes)
    one = MeshExtractor(dec, 64, 64)
    assert len(got) == len(codes)
    for c, m in zip(codes, got):
        ref = one.extract_mesh_from_code(c)
        assert np.array_equal(m.vertices, ref.vertices) and np.array_equal(m.faces, ref.faces)


def test_remesh_map_prepass_tool(tmp_path, mirror):
    import json
    import runpy
    from dsp_slam_amd.map_objects import read_map_objects, write_map_objects
    from reconstruct.utils import read_mesh_from_ply
    g = golden("golden_map_objects.npz")
    cars = fixtures.materialize_decoder_dir("cars", str(tmp_path / "cars_64"))
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    cfg["DeepSDF_DIR"] = cars
    cfg.setdefault("data_type", "KITTI")
    cfg_path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(cfg_path, "w"))
    dirs = {}
    for mode in ("off", "f16"):
        d = tmp_path / mode
        d.mkdir()
        with open(d / "MapObjects.txt", "wb") as f:
            f.write(g["text"].tobytes())
        objs = read_map_objects(str(d / "MapObjects.txt"))
        for o, c3 in zip(objs[:3], ((0.3, -0.2, 0.1), (-0.4, 0.5, 0.0), (0.25, -0.1, 0.05))):
            o["code"] = np.zeros(64, np.float32)
            o["code"][:3] = c3
        write_map_objects(str(d / "MapObjects.txt"), objs)
        old = sys.argv
        sys.argv = ["remesh_map.py", "--config", cfg_path, "--map_dir", str(d), "--voxels_dim", "48", "--prepass", mode]
        try:
            runpy.run_path(os.path.join(ROOT, "tools", "remesh_map.py"), run_name="__main__")
        finally:
            sys.argv = old
        dirs[mode] = d / "objects"
    plys = sorted(p for p in os.listdir(dirs["off"]) if p.endswith(".ply"))
    assert len(plys) >= 2 and plys == sorted(p for p in os.listdir(dirs["f16"]) if p.endswith(".ply"))
    for p in plys:
        v0, f0 = read_mesh_from_ply(str(dirs["off"] / p))
        v1, f1 = read_mesh_from_ply(str(dirs["f16"] / p))
        assert np.array_equal(v0, v1) and np.array_equal(f0, f1)
        assert open(dirs["off"] / p, "rb").read() == open(dirs["f16"] / p, "rb").read()
    assert not any(p.endswith("_sdf.npy") for p in os.listdir(dirs["f16"]))
