"""GPU: the throughput form of the fp32 decoder (mlp_kernel<0..3>) across its output-group boundaries.

The kernel hides each boundary's work -- the read-out of the finished group's accumulators and the bias seed of the group after the next
-- behind the MFMAs of the following group's first chunk, on two alternating accumulator sets.  A slip there (a set seeded before it was
read out, a seed taken from the wrong group or the wrong vector, ring state lost across a tile) changes bits, so the throughput form is
compared BIT FOR BIT with the latency form (mlp_split_kernel), which shares the arithmetic and none of that schedule; the oracle
comparison keeps the tolerances of tests/test_gpu_decoders.py.

Sizes: 1 / 16 / 63 / 64 / 65 / 129 points = one valid lane, one wave, a tile short of one point, a full tile, a second tile with one
valid point, three tiles (the prefetch wraps a tile boundary, the ring state carries over); both fixture decoders: cars (64-D codes,
latent_in layer of 7 chunks, 7-group layer in front of it) and chairs32 (32-D codes: the other lat_tile)."""
import numpy as np
import pytest

import launch_forms as F
from dsp_slam_amd import _lib as L, engine as E, synth
from oracle import dsp_oracle as O

pytestmark = pytest.mark.gpu

COUNTS = (1, 16, 63, 64, 65, 129)
N_DEPTH = 8
N_FG, N_BG = 30, 10           # 40 rays per object
TRACE_KEYS = ("H", "b", "dx", "V", "K", "set_sums", "t_obj_cam", "code")
COUNT_KEYS = ("n_fwd_points", "n_jac_points", "n_render_rows")
# mask reuse on / off -> pins of the throughput form and of the latency form with the same reuse
THROUGHPUT = {True: dict(F.FORMS["throughput"]["pins"]), False: dict(split_rows=0, mask_reuse=0, wave_bookkeeping=0)}
# (the speculative band off in both: it would send the band's rows through the jacobian launch instead of the forward launch, and the
# point counts of the two forms are compared launch for launch)
LATENCY = {True: dict(F.FORMS["mixed_reuse"]["pins"], cluster_tiles=0), False: dict(F.FORMS["split_rows"]["pins"], cluster_tiles=0, speculative_band=0)}


@pytest.fixture(scope="module")
def decoders(oracle_decoder, chairs32_decoder):
    return dict(cars=oracle_decoder, chairs32=chairs32_decoder)


@pytest.fixture(scope="module")
def engines(decoders):
    out = {k: E.Engine(d.layers, d.latent_in, d.code_len, device=0) for k, d in decoders.items()}
    yield out
    for e in out.values():
        e.close()


def _object(fixture, seed, n_surface):
    kw = dict(code_len=32, half=synth.CHAIR_HALF) if fixture == "chairs32" else {}
    return synth.make_object(seed, n_surface=n_surface, n_background=N_BG, n_foreground=N_FG, **kw)


def _plan(objs, pins, prepass):
    return F.plan_of(F.shape_of(F.sizes(objs), N_DEPTH), dict(pins, prepass=prepass))


def _run(eng, objs, n_it, pins, prepass):
    """-> (result and trace arrays by name, stats) of the batch run with `pins` set."""
    prm = E.gn_params(num_iterations=n_it, num_depth_samples=N_DEPTH)
    b = eng.batch(prm, [o["t_cam_obj_init"] for o in objs], [o["pts"] for o in objs], [o["rays"] for o in objs], [o["depth"] for o in objs], trace=True)
    F.pin(b, dict(pins, prepass=prepass))
    b.run()
    out = dict(zip(("t_cam_obj", "code", "loss", "status"), b.results()))
    for e in range(n_it):
        tr = b.trace(e)
        out.update({"trace[%d].%s" % (e, k): tr[k] for k in TRACE_KEYS})
    st = b.stats()
    b.close()
    return out, st


def _assert_same_bits(what, got, ref):
    assert list(got) == list(ref)
    for k in ref:
        a, c = np.asarray(got[k]), np.asarray(ref[k])
        same = np.array_equal(a, c) or np.array_equal(a.view(np.uint8), c.view(np.uint8))        # (the second: NaNs of the same bits)
        assert same, "%s: %s differs in %d of %d entries" % (what, k, (a != c).sum(), a.size)


def _throughput_against_latency(eng, objs, n_it, reuse, prepass):
    tp, lat = _plan(objs, THROUGHPUT[reuse], prepass), _plan(objs, LATENCY[reuse], prepass)
    # the pins reach the forms they name: 64-point tiles of the throughput kernels everywhere / the latency form's row split, no cluster tiles
    assert tp["split_rows"] == 0 and tp["split_fwd"] == 0 and tp["cluster"] == 0 and tp["jac_tile_pts"] == 64 and tp["fwd_tile_pts"] == 64, tp
    assert tp["mask_reuse"] == int(reuse) and tp["reuse_throughput"] == int(reuse), tp
    assert lat["split_rows"] == 1 and lat["reuse_throughput"] == 0 and lat["cluster"] == 0 and lat["jac_tile_pts"] == 16 and lat["mask_reuse"] == int(reuse), lat
    assert tp["prepass_mode"] == lat["prepass_mode"] == int(prepass != L.PREPASS_OFF)
    got, st = _run(eng, objs, n_it, THROUGHPUT[reuse], prepass)
    ref, st_ref = _run(eng, objs, n_it, LATENCY[reuse], prepass)
    what = "reuse %d prepass %d" % (reuse, prepass)
    print(what, "counts", {k: (st[k], st_ref[k]) for k in COUNT_KEYS}, "V", got["trace[0].V"].tolist(), "K", got["trace[0].K"].tolist(), "status", got["status"].tolist())
    assert st["prepass_guard_rerun"] == 0 and st_ref["prepass_guard_rerun"] == 0
    assert (st["n_render_rows"] > 0) == reuse and st["n_jac_points"] > 0 and st["n_fwd_points"] > 0, st
    _assert_same_bits(what, got, ref)
    for k in COUNT_KEYS:
        assert st[k] == st_ref[k], (what, k, st[k], st_ref[k])
    return got


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("fixture", ["cars", "chairs32"])
def test_decode_and_jacobian_on_few_points(engines, decoders, fixture, n):
    eng, dec = engines[fixture], decoders[fixture]
    rng = np.random.default_rng(1000 * n + dec.code_len)
    code = (rng.normal(size=dec.code_len) * 0.2).astype(np.float32)
    pts = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    # mlp_kernel<0> and <2> against the oracle, as tests/test_gpu_decoders.py holds them
    y, gr = O.get_batch_sdf_jacobian(dec, code, pts)
    assert np.abs(eng.decode_sdf(code, pts) - O.decode_sdf(dec, code, pts)).max() < 5e-6
    s2, g2 = eng.sdf_jacobian(code, pts)
    assert g2.shape == (n, dec.code_len + 3)
    d = np.abs(g2 - gr).max(1)
    print("max |sdf - oracle| %.2e, max |grad - oracle| %.2e of %.2e" % (np.abs(s2 - y).max(), d.max(), np.abs(gr).max()))
    assert np.abs(s2 - y).max() < 5e-6 and (d < 1e-5 * max(1.0, np.abs(gr).max())).mean() >= 0.999 and d.max() < 2e-2
    # the same kernels on n surface points (and 40 rays) of one object, against the latency form, bit for bit
    obj = _object(fixture, 900 + n, n)
    assert obj["pts"].shape[0] == n and obj["rays"].shape[0] == N_FG + N_BG
    _throughput_against_latency(eng, [obj], 1, False, L.PREPASS_OFF)


@pytest.mark.parametrize("prepass", [L.PREPASS_OFF, L.PREPASS_F16])
@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("fixture", ["cars", "chairs32"])
def test_all_four_modes_through_a_batch(engines, fixture, reuse, prepass):
    """reuse on: mlp_kernel<1> exports the masks of the band, <3> takes the render rows from them and <2> the surface rows; reuse off: <2>
    takes the render rows too (forward launches: <1> / <0>)."""
    objs = [_object(fixture, 950 + i, 65) for i in range(2)]
    got = _throughput_against_latency(engines[fixture], objs, 2, reuse, prepass)
    assert got["status"].tolist() == [0, 0] and all((got["trace[%d].K" % e] > 0).all() for e in range(2))
