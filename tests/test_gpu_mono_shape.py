"""GPU: the monocular input shape, n_fg != M (reference src/LocalMapping_util.cc:330-392) -- M valid map points on the object, n_fg
feature rays of the detection that carry a depth, the two independent -- in a ragged batch whose depth_off and pts_off run apart.

One 16-object batch from synth.make_object(..., n_foreground=k): M from 50 to 400, k / M from 0 (all background) to 1.5, one object with
no background ray at all (k = n_rays).  Every traced iteration of every object against the oracle at the device's own state
(tests/test_gpu_parity.py::_check_iterations); every object's result equal to its single-object run, bit for bit; the whole batch
bit-identical across the launch forms and prepass modes the library chooses between; the low-precision compute mode runs and stays within
the bounds tests/test_gpu_lp_compute.py holds it to.  (The recorded reference runs of this shape, golden_recon_mono_*.npz, are in
tests/test_gpu_forensics.py's CASES.)
"""
import numpy as np
import pytest

import test_gpu_parity as P
from oracle import dsp_oracle as O
from dsp_slam_amd import engine as E, synth, _lib as L

pytestmark = pytest.mark.gpu

N_IT = 3
# (m is not compared: which samples behind a solid one get decoded depends on the form, tests/test_gpu_prepass.py)
TRACE_KEYS = ("H", "b", "dx", "V", "K", "set_sums", "t_obj_cam", "code", "depths")


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _objects():
    m = np.linspace(50, 400, 16).round().astype(int)
    ratio = np.linspace(0.0, 1.5, 16)
    objs = []
    for i in range(16):
        n_bg = 0 if i == 15 else 60 + 10 * i             # the last: k = n_rays, no background ray
        objs.append(synth.make_object(6100 + i, n_surface=int(m[i]), n_background=n_bg, n_foreground=int(round(ratio[i] * m[i]))))
    return objs


def _args(objs):
    return ([o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs])


def _run(eng, prm, objs, **setters):
    b = eng.batch(prm, *_args(objs), trace=True)
    for k, v in setters.items():
        if isinstance(v, tuple):
            getattr(b, "set_" + k)(*v)
        else:
            getattr(b, "set_" + k)(v)
    b.run()
    out = (b.results(), [b.trace(e) for e in range(N_IT)], b.stats())
    b.close()
    return out


def _same(a, c, what, rows=slice(None)):
    for x, y in zip(a[0], c[0]):
        assert np.array_equal(x[rows], y[rows], equal_nan=True), what
    for e, (ta, tc) in enumerate(zip(a[1], c[1])):
        for k in TRACE_KEYS:
            assert np.array_equal(ta[k][rows], tc[k][rows]), (what, e, k)


@pytest.fixture(scope="module")
def batch(eng):
    objs = _objects()
    n_fg = [o["depth"].shape[0] for o in objs]
    m = [o["pts"].shape[0] for o in objs]
    assert n_fg[0] == 0 and objs[15]["rays"].shape[0] == n_fg[15] and n_fg[15] > m[15]
    assert sum(a != b for a, b in zip(n_fg, m)) >= 15
    prm = E.gn_params(num_iterations=N_IT)
    return objs, prm, _run(eng, prm, objs)


def test_every_iteration_against_the_oracle(eng, oracle_decoder, batch):
    """tests/test_gpu_parity.py::_check_iterations for every object, with one refinement of its fp64 entry check: at a state where the fp32
    ORACLE's own system is outside TAU of the fp64 linearisation (measured once here: the no-background object's second iteration, 28 render
    rows with a hidden ReLU within round-off of zero; the oracle's H_code block is 5.50e-3 from fp64, the device's 5.49e-3), the device must
    be no further from fp64 than the oracle, block for block (10 % slack); everywhere else it must be within TAU."""
    import gn_metric as M
    objs, prm, (res, traces, _) = batch
    assert (res[3] == 0).all(), res[3]
    oprm = O.GNParams(num_iterations=N_IT)
    beyond, named = [], []
    for i, o in enumerate(objs):
        tr_i = [{k: v[i:i + 1] for k, v in tr.items()} for tr in traces]
        for e, tr in enumerate(tr_i):
            it, itj, own, lin = P.one_iteration_oracle(oracle_decoder, oprm, o, tr)
            P.compare_linearisation(tr, 0, (it, itj, own), oprm.k4)        # the max-norm bounds (asserted inside)
            if not P.LAST_LINEARISATION["same_sets"]:
                P.explain_flips(eng, prm, oprm, oracle_decoder, o, tr)        # every differing sample named, within round-off
                named.append((i, e))
                continue
            dev = M.scaled_errors(dict(H=tr["H"][0], b=tr["b"][0], dx=tr["dx"][0]), lin, oprm.k4, (it, itj))
            ora = M.scaled_errors(it, lin, oprm.k4)
            if M.within_tau(ora):
                M.assert_within_tau(dev, "object %d iteration %d" % (i, e))
            else:
                beyond.append((i, e, M.flat(ora)))
                fd, fo = M.flat(dev), M.flat(ora)
                assert all(fd[k] <= max(1.1 * fo[k], M.TAU_H if k.startswith("H_") else M.TAU_B) for k in fd if k != "solve"), (i, e, fd, fo)
                assert fd["solve"] <= M.TAU_SOLVE
    print("states where the fp32 oracle itself is outside TAU of fp64: %s" % beyond)
    assert len(beyond) <= 2, beyond
    assert len(named) <= 1, named          # _check_iterations allows one iteration with named flips per object; measured: none


def test_each_object_equals_its_single_run(eng, batch):
    objs, prm, full = batch
    for i, o in enumerate(objs):
        one = _run(eng, prm, [o])
        for x, y in zip(one[0], full[0]):
            assert np.array_equal(x[0], y[i], equal_nan=True), i
        for e in range(N_IT):
            for k in TRACE_KEYS:
                assert np.array_equal(one[1][e][k][0], full[1][e][k][i]), (i, e, k)
        if i % 5 == 0:          # a one-object batch may skip the tile lists (direct tiles): the same bits either way
            _same(one, _run(eng, prm, [o], direct_tiles=0), "object %d, direct tiles off" % i)
            _same(one, _run(eng, prm, [o], direct_tiles=1), "object %d, direct tiles on" % i)


@pytest.mark.parametrize("form", ["cluster_off", "cluster_on", "split_rows", "wave_off", "wave_on", "prepass_off_one_pass", "prepass_f16", "prepass_bf16"])
def test_launch_forms_and_prepass_modes_are_bit_identical(eng, batch, form):
    objs, prm, ref = batch
    setters = dict(cluster_off=dict(cluster_tiles=0), cluster_on=dict(cluster_tiles=1), split_rows=dict(split_rows=1, mask_reuse=0),
                   wave_off=dict(wave_bookkeeping=0), wave_on=dict(wave_bookkeeping=1), prepass_off_one_pass=dict(prepass=L.PREPASS_OFF, ray_passes=1),
                   prepass_f16=dict(prepass=L.PREPASS_F16, prepass_guard=True), prepass_bf16=dict(prepass=L.PREPASS_BF16, prepass_guard=True))[form]
    run = _run(eng, prm, objs, **setters)
    _same(run, ref, form)
    if form.startswith("prepass_f") or form.startswith("prepass_b"):
        assert run[2]["prepass_guard_trips"] == 0 and run[2]["n_mlp_prepass_launches"] > 0


def test_low_precision_compute_mode_runs(eng, batch):
    """Not a parity path: it runs, every object ends good, and its first iteration -- from the same state as the fp32 path's -- has the same
    in-sphere set and a kept set, H and loss within the f16 bounds of tests/test_gpu_lp_compute.py (|dK| <= 5 % of K, rel dH <= 5 %)."""
    objs, prm, ref = batch
    run = _run(eng, prm, objs, compute=L.COMPUTE_F16, lp_small_batches=1)
    assert (run[0][3] == 0).all()
    assert run[2]["n_mlp_fwd_launches"] == 0
    t0, r0 = run[1][0], ref[1][0]
    for i in range(len(objs)):
        assert np.array_equal(t0["t_obj_cam"][i], r0["t_obj_cam"][i])
        assert int(t0["V"][i]) == int(r0["V"][i]), i
        assert abs(int(t0["K"][i]) - int(r0["K"][i])) <= 0.05 * max(int(r0["K"][i]), 1), (i, int(t0["K"][i]), int(r0["K"][i]))
        assert P.rel(t0["H"][i], r0["H"][i]) <= 0.05, (i, P.rel(t0["H"][i], r0["H"][i]))
