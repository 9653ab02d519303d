"""GPU: the multi-view path (dsp_batch_create_multiview, k_group_reduce, k_group_broadcast, k_solve's pooled divisors) held entry by entry
to the pooled fp64 linearisation (oracle.dsp_oracle.linearise_fp64_multiview, tests/gn_metric.py), at the device's own states.

Every iteration of every case: the composed fp32 oracle (tests/multiview_oracle.py), its sdf-jitter twin and the pooled fp64 system are
evaluated at the device's traced state on the device's per-view depth samples; then
  * the device's depths lie within 2.5 ulp of the oracle's own derivation, and every view's T_oc_v is the oracle's bit for bit;
  * per-view (V, K) and both set checksums are the oracle's; the pooled V and K are the sums (the pooled M is fixed by the inputs and
    reaches the trace only as H's surface part: the metric sees a wrong divisor through Ds);
  * H, b and dx are within TAU_H / TAU_B / TAU_SOLVE of the pooled fp64 (check_against_fp64 with the jitter twin's allowance), BESIDE the
    max-norm bounds of tests/test_gpu_multiview.py, which stay;
  * the measured scaled errors go to parity_log(kind="multiview_fp64").
An iteration in which a view's checksums differ from the oracle's is held to compare_linearisation's loose bound instead -- at most one per
case, and only when every differing sample is named (Batch.debug_samples takes the view's row: a view is a batch row) and lies within
round-off of the threshold it crossed.

Cases (inputs: tests/multiview_metric.py; their conditions -- transitions, jitter-stable sets -- are asserted on the CPU in
tests/test_multiview_metric.py): three views; a ragged batch of 2-, 1- and 3-view objects in two orders; a view that joins late; a view
whose render rows vanish while it stays in the sphere; a view with V < 10 beside a good one and an all-away neighbour; 33 and 64 depth
samples; the chairs32 decoder (39 x 39 system); the reference's recorded states.
"""
import json

import numpy as np
import pytest

import forensics as F
import gn_metric as M
import multiview_metric as X
import multiview_oracle as MV
from conftest import golden, parity_log
from dsp_slam_amd import _lib as L, engine as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(oracle_decoder, chairs32_decoder):
    made = {}

    def get(kind):
        if kind not in made:
            dec = chairs32_decoder if kind == "chairs32" else oracle_decoder
            made[kind] = (dec, E.Engine(dec.layers, dec.latent_in, dec.code_len, device=0))
        return made[kind]
    yield get
    for _, e in made.values():
        e.close()


def engine_params(case):
    return E.gn_params(num_iterations=case["n_it"], num_depth_samples=case["n_depth"], cut_off=case["cut_off"], **X.HYPER)


def run_traced(eng, case, order=None):
    """Run the case's objects (in `order`) as one traced batch -> (results, [(trace, trace_views) per iteration], row offsets per object)."""
    objs = [case["objects"][i] for i in (order or range(len(case["objects"])))]
    b = eng.multiview_batch(engine_params(case), [o["t"] for o in objs], [o["views"] for o in objs], trace=True)
    b.run()
    res = b.results()
    traces = [(b.trace(e), b.trace_views(e)) for e in range(case["n_it"])]
    b.close()
    return res, traces, np.concatenate([[0], np.cumsum([len(o["views"]) for o in objs])]).astype(int)


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def view_flips(eng, case, obj, tr, tv, i, rows, it, which):
    """Re-run the one iteration from the traced state as a batch of this object alone and compare the device's per-sample decisions of the
    views `which` (Batch.debug_samples by the view's row) with the oracle's sets -> {view: [named flips]} (tests/forensics.py)."""
    n_d = case["n_depth"]
    b = eng.multiview_batch(engine_params(case), [obj["t"]], [obj["views"]], trace=True)
    b.set_start_state([tr["t_obj_cam"][i]], [tr["code"][i]], tv["depths"][rows])
    b.set_iterations(1)
    b.run()
    assert np.array_equal(b.trace_views(0)["set_sums"], tv["set_sums"][rows]), "the re-run from the traced state does not reproduce the traced sets"
    out = {}
    for k in which:
        assert it["views"][k]["sets"] is not None, "view %d: the oracle has no render term here" % k
        n_rays = obj["views"][k]["rays"].shape[0]
        m, sdf, deds = b.debug_samples(k, n_rays, n_d)
        out[k] = F.name_flips(m, sdf, deds, F.oracle_grids(it["views"][k]["sets"], n_rays, n_d), case["cut_off"])
    b.close()
    return out


def name_view_flips(eng, case, obj, tr, tv, i, rows, it, differing):
    """Every sample of the views `differing` on which the device and the oracle decided differently, named; each must lie within round-off
    of the threshold it crossed."""
    named = []
    for k, flips in view_flips(eng, case, obj, tr, tv, i, rows, it, differing).items():
        assert flips, "view %d: the checksums differ but no differing sample was found" % k
        assert all(f["explained"] for f in flips), flips
        named += [dict(f, view=k) for f in flips]
    return named


def check_iteration(eng, dec, case, label, obj, tr, tv, i, rows, e, given_depths=None):
    """One iteration of object i (view rows `rows` of the batch) against the oracle at the device's own state.  -> True when the strict
    comparison was made, False when the iteration went the loose way."""
    oprm = X.oracle_params(case)
    n_d, n = case["n_depth"], X.PD + case["code_len"]
    t, code = tr["t_obj_cam"][i], tr["code"][i][:case["code_len"]]
    assert np.all(tr["code"][i][case["code_len"]:] == 0) and np.all(tr["dx"][i][n:] == 0)
    depths = tv["depths"][rows, :n_d]
    for k, view in enumerate(obj["views"]):
        t_v, own = MV.view_state(t, view["t_ref_cam"], n_d)
        assert np.array_equal(tv["t_obj_cam"][rows][k], t_v), "view %d: T_oc_v is not the fp64 product rounded once" % k
        want = own if given_depths is None else np.asarray(given_depths[k], np.float32)[:n_d]
        tol = 2.5 * np.spacing(np.abs(own).max()) if given_depths is None else 0.0
        assert np.abs(depths[k] - want).max() <= tol, "view %d: depth samples" % k
    lins = X.linearise_at(dec, oprm, obj["views"], t, code, depths)
    assert lins is not None, "the composed oracle has no linearisation at the device's state"
    it, itj, lin = lins
    dev_vk = [(int(v), int(k)) for v, k in zip(tv["V"][rows], tv["K"][rows])]
    differing = [k for k, v in enumerate(it["views"]) if (int(tv["set_sums"][rows][k][0]), int(tv["set_sums"][rows][k][1])) != (v["vsum"], v["ksum"])]
    dev = dict(H=tr["H"][i][:n, :n], b=tr["b"][i][:n], dx=tr["dx"][i][:n])
    hs, bs = np.abs(it["H"]).max(), np.abs(it["b"]).max()
    mask = np.ones(n, bool)
    mask[3:6] = False                  # b[3:6] carries the rotation prior's quantised residual (MV.rot_prior_bound)
    rel_h, rel_b = float(np.abs(dev["H"] - it["H"]).max() / hs), float(np.abs(dev["b"] - it["b"])[mask].max() / bs)
    print("%s iteration %d: (V, K) device %s oracle %s; max-norm rel dH %.3e db %.3e (b outside 3:6)" % (label, e, dev_vk, X.view_vk(it), rel_h, rel_b))
    assert int(tr["V"][i]) == sum(v for v, _ in dev_vk) and int(tr["K"][i]) == sum(k for _, k in dev_vk)
    assert it["M"] == lin["N"] == sum(v["pts"].shape[0] for v in obj["views"])
    if differing:
        named = name_view_flips(eng, case, obj, tr, tv, i, rows, it, differing)
        flips = sum(abs(d[0] - o[0]) + abs(d[1] - o[1]) for d, o in zip(dev_vk, X.view_vk(it)))
        print("%s iteration %d: views %s select other sets than the oracle: %s" % (label, e, differing, named))
        assert flips <= max(4, it["K"] // 250)
        loose = 8.0 * max(flips, 2) / max(it["K"], 1)
        assert np.abs(dev["H"] - it["H"]).max() < loose * hs + 4 * np.abs(itj["H"] - it["H"]).max()
        assert np.abs(dev["b"] - it["b"])[mask].max() < loose * bs + 4 * np.abs(itj["b"] - it["b"])[mask].max()
        parity_log(kind="multiview_fp64", case=label, iteration=e, same_sets=False, flips=named, rel_H=rel_h, rel_b=rel_b)
        return False
    assert X.same_sets(it, itj), "%s iteration %d: the jitter twin selects other sets at the device's state" % (label, e)
    assert dev_vk == X.view_vk(it)
    assert int(tr["K"][i]) == it["K"] == lin["K"] and lin["K_views"] == [k for _, k in dev_vk]
    rd = M.scaled_errors(dev, lin, oprm.k4, (it, itj))
    print("%s iteration %d: scaled error against the pooled fp64: %s" % (label, e, M.flat(rd)))
    rec = M.check_against_fp64(dev, lin, oprm.k4, pair=(it, itj), what="%s iteration %d" % (label, e))
    parity_log(kind="multiview_fp64", case=label, iteration=e, same_sets=True, V=[v for v, _ in dev_vk], K=[k for _, k in dev_vk], rel_H=rel_h, rel_b=rel_b, **rec)
    assert X.max_norm_passes(dev, it, oprm.k4), (label, e, rel_h, rel_b)
    return True


def check_object(eng, dec, case, label, traces, off, pos, obj):
    """Every iteration of the object at position `pos` of the batch; at most one may go the loose way."""
    rows = slice(int(off[pos]), int(off[pos + 1]))
    strict = [check_iteration(eng, dec, case, label, obj, tr, tv, pos, rows, e) for e, (tr, tv) in enumerate(traces)]
    assert strict.count(False) <= 1, "%s: %d iterations with sets that differ from the oracle's" % (label, strict.count(False))


# ---------------------------------------------------------------------------------------------------------------------------------------
# a, c, d, f, g: one object
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_views", "late_join", "leaving", "depth33", "depth64", "chairs32"])
def test_one_object_every_iteration_within_tau_of_the_pooled_fp64(engines, name):
    case = X.CASES[name]()
    dec, eng = engines(case["decoder"])
    res, traces, off = run_traced(eng, case)
    assert res[3].tolist() == [0]
    assert res[1].shape == (1, case["code_len"])
    check_object(eng, dec, case, name, traces, off, 0, case["objects"][0])
    vk = [(int(tv["V"][-1]), int(tv["K"][-1])) for _, tv in traces]              # the last view: the one a transition case is about
    if case.get("transition") == "join":
        # its rows enter the pooled sums in an iteration that was checked above, and stay
        first = min(e for e, (v, k) in enumerate(vk) if k > 0)
        assert vk[0][0] < 10 and 0 < first < case["n_it"] - 1
    if case.get("transition") == "leave":
        # once its K is 0 (V still >= 10) the pooled K is the other view's: its render Gram is absent from the pooled system (through Dr above)
        gone = [e for e, (v, k) in enumerate(vk) if k == 0]
        assert vk[0][1] > 0 and len(gone) >= 2 and all(vk[e][0] >= 10 for e in gone)
        assert all(int(traces[e][0]["K"][0]) == int(traces[e][1]["K"][0]) for e in gone)


def test_a_view_is_a_batch_row_for_debug_samples(engines):
    """What the loose path relies on to name flips: Batch.debug_samples by a view's row gives that view's decisions.  Where the checksums
    agree with the oracle's, the per-sample grids of every view with a render term do too -- in the iteration the late view's rows first
    enter (its 24 rays are not the leader's 190)."""
    case = X.case_late_join()
    dec, eng = engines("cars")
    _, traces, off = run_traced(eng, case)
    obj, rows = case["objects"][0], slice(0, 2)
    e = min(e for e, (_, tv) in enumerate(traces) if int(tv["K"][1]) > 0)
    tr, tv = traces[e]
    it, _, _ = X.linearise_at(dec, X.oracle_params(case), obj["views"], tr["t_obj_cam"][0], tr["code"][0][:64], tv["depths"][rows, :case["n_depth"]], fp64=False)
    assert [(int(tv["set_sums"][k][0]), int(tv["set_sums"][k][1])) for k in range(2)] == [(v["vsum"], v["ksum"]) for v in it["views"]]
    assert view_flips(eng, case, obj, tr, tv, 0, rows, it, [0, 1]) == {0: [], 1: []}


# ---------------------------------------------------------------------------------------------------------------------------------------
# b: a ragged batch, in two orders
# ---------------------------------------------------------------------------------------------------------------------------------------
RAGGED_ORDERS = ([0, 1, 2], [2, 0, 1])


@pytest.fixture(scope="module")
def ragged(engines):
    case = X.case_ragged()
    _, eng = engines("cars")
    return case, [run_traced(eng, case, order) for order in RAGGED_ORDERS]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_ragged_batch_every_object_within_tau_of_the_pooled_fp64(engines, ragged, i):
    """Objects of 2, 1 and 3 views: a group whose leader is not row 0, and a one-member group between larger ones."""
    case, runs = ragged
    dec, eng = engines("cars")
    (res, traces, off), (res2, traces2, _) = runs
    assert res[3].tolist() == [0, 0, 0] and res2[3].tolist() == [0, 0, 0]
    check_object(eng, dec, case, "ragged object %d (%d views)" % (i, len(case["objects"][i]["views"])), traces, off, i, case["objects"][i])
    # the same batch in the order [2, 0, 1]: the same bits per object, results and every iteration's system
    p = RAGGED_ORDERS[1].index(i)
    assert same_bits([x[i] for x in res], [x[p] for x in res2])
    for (tr, _), (tr2, _) in zip(traces, traces2):
        assert same_bits([tr[k][i] for k in ("H", "b", "dx", "V", "K", "t_obj_cam", "code")], [tr2[k][p] for k in ("H", "b", "dx", "V", "K", "t_obj_cam", "code")])


# ---------------------------------------------------------------------------------------------------------------------------------------
# e: a view with V < 10 beside a good one; a neighbour with away views only
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_away_view_beside_a_good_one_and_an_all_away_neighbour(engines):
    case = X.case_away()
    dec, eng = engines("cars")
    res, traces, off = run_traced(eng, case)
    assert res[3].tolist() == [0, L.OBJ_FEW_SAMPLES]
    check_object(eng, dec, case, "away_view", traces, off, 0, case["objects"][0])
    for tr, tv in traces:
        assert int(tv["V"][1]) < 10 and int(tv["K"][1]) == 0 and int(tr["K"][0]) == int(tv["K"][0])
    alone = dict(case, objects=case["objects"][:1])
    res1, traces1, _ = run_traced(eng, alone)
    assert same_bits([x[0] for x in res], [x[0] for x in res1]), "the all-away neighbour changed the object's bits"
    for (tr, _), (tr1, _) in zip(traces, traces1):
        assert same_bits([tr[k][0] for k in ("H", "b", "dx")], [tr1[k][0] for k in ("H", "b", "dx")])


# ---------------------------------------------------------------------------------------------------------------------------------------
# h: the reference's recorded states
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0, 4, 9])
def test_reference_recorded_states_within_tau_of_the_pooled_fp64(engines, e):
    g = golden("golden_multiview_cars3.npz")
    cfg = json.loads(str(g["cfg_json"]))
    o, j = cfg["optimizer"], cfg["optimizer"]["joint_optim"]
    assert {k: j[k] for k in ("k1", "k2", "k3", "k4", "b1", "b2")} == {k: X.HYPER[k] for k in ("k1", "k2", "k3", "k4", "b1", "b2")}
    assert (j["learning_rate"], j["scale_damping"], o["code_len"]) == (X.HYPER["lr"], X.HYPER["s_damp"], 64)
    obj = dict(t=g["in_t_cam_obj_init"], views=MV.golden_views(g))
    case = X._case([obj], 1, n_depth=o["num_depth_samples"], cut_off=o["cut_off_threshold"])
    dec, eng = engines("cars")
    b = eng.multiview_batch(engine_params(case), [obj["t"]], [obj["views"]], trace=True)
    b.set_start_state([g["it_t_obj_cam"][e]], [g["it_code"][e]], g["it_depths"][e])
    b.run()
    assert b.results()[3][0] == 0
    tr, tv = b.trace(0), b.trace_views(0)
    b.close()
    assert np.array_equal(tr["t_obj_cam"][0], g["it_t_obj_cam"][e]) and np.array_equal(tr["code"][0], g["it_code"][e])
    assert tv["V"].tolist() == g["it_V"][e].tolist() and tv["K"].tolist() == g["it_K"][e].tolist()
    strict = check_iteration(eng, dec, case, "golden_multiview_cars3", obj, tr, tv, 0, slice(0, len(obj["views"])), e, given_depths=g["it_depths"][e])
    assert strict, "the device selects other sets than the oracle at a recorded state"
