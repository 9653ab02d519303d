"""CPU: the pooled fp64 linearisation (oracle.dsp_oracle.linearise_fp64_multiview) and the entry-by-entry metric (tests/gn_metric.py) on
multi-view Gauss-Newton systems.

  * identity: one identity view IS linearise_fp64, bit for bit, at recorded single-view states; the parts add up to H and b;
  * sanity: at all ten recorded iterations of tests/golden/golden_multiview_cars3.npz the composed fp32 oracle, its sdf-jitter twin and the
    reference's own recorded system are within TAU of the pooled fp64; per-view V, K and checksums are the recorded ones;
  * every case tests/test_gpu_multiview_metric.py uses (tests/multiview_metric.py): each iteration of the composed oracle's own run is within
    TAU of the pooled fp64, selects the same sets as its jitter twin, and shows the transition the case was built for.  These are
    conditions on the INPUTS of the GPU tests: a seed that breaks one is replaced here;
  * power: six faults of a member view on its way into the leader's sums, built at the level of that view's rows, at two states each of a
    3-view and a 4-view object: the unperturbed system is accepted, the first five are rejected at every state (the max-norm bound of
    tests/test_gpu_multiview.py passes the first two).  What the max-norm bound says is printed, not asserted.  "Three render rows lost"
    is printed only: measured 1.8e-3 / 1.1e-3 on the 3-view object but 1.6e-4 / 6.8e-4 on the 4-view one (accepted at its iteration 1).
    The x 1.01 fault sits AT TAU_H on four-view objects (tests/multiview_metric.py, FAULT_OBJECTS): rejected here, not on every seed.
"""
import json

import numpy as np
import pytest

import gn_metric as M
import multiview_metric as X
import multiview_oracle as MV
from conftest import golden
from oracle import dsp_oracle as O
from test_gn_metric import _state

EYE = np.eye(4, dtype=np.float32)
_FAULT_STATES = []


def _dec(case, oracle_decoder, chairs32_decoder):
    return chairs32_decoder if case["decoder"] == "chairs32" else oracle_decoder


def _parts_add_up(lin):
    assert np.array_equal(lin["Dr"] + lin["Ds"] + lin["H_code_prior"] + lin["H_rot"] + lin["H_damp"], lin["H"])
    assert np.array_equal(lin["gr"] + lin["gs"] + lin["b_code_prior"] + lin["b_rot"], lin["b"])


@pytest.mark.parametrize("name,which", [("golden_recon_small.npz", 0), ("golden_recon_chairs32.npz", -1)])
def test_one_identity_view_is_linearise_fp64(name, which):
    prm, dec, inputs, state, ref, it, lin = _state(name, which)
    view = dict(t_ref_cam=EYE, pts=inputs[0], rays=inputs[1], depth=inputs[2])
    got = O.linearise_fp64_multiview(dec, prm, [view], state[0], state[1], [state[2]], [it["sets"]])
    for k in ("H", "b", "dx", "Dr", "Ds", "gr", "gs", "Lr", "Ls", "H_flip", "b_flip"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(lin[k])), k
    assert (got["V"], got["K"], got["N"], got["n_flip"]) == (lin["V"], lin["K"], lin["N"], lin["n_flip"])
    assert (got["V_views"], got["K_views"], got["N_views"]) == ([lin["V"]], [lin["K"]], [lin["N"]])
    _parts_add_up(got)


def test_a_view_without_rows_does_not_divide_by_zero(oracle_decoder):
    """A view without points and with an empty `kept` set changes nothing; without any render row or any point the term is absent, not NaN."""
    prm, dec, inputs, state, ref, it, lin = _state("golden_recon_small.npz", 0)
    view = dict(t_ref_cam=EYE, pts=inputs[0], rays=inputs[1], depth=inputs[2])
    empty = dict(t_ref_cam=EYE, pts=np.zeros((0, 3), np.float32), rays=inputs[1][:5], depth=np.zeros(0, np.float32))
    with np.errstate(all="raise"):
        got = O.linearise_fp64_multiview(dec, prm, [view, empty], state[0], state[1], [state[2], state[2]], [it["sets"], None])
        for k in ("H", "b", "dx", "Dr", "Ds", "gr", "gs", "Lr", "Ls", "H_flip", "b_flip"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(lin[k])), k
        assert got["K_views"] == [lin["K"], 0] and got["N_views"] == [lin["N"], 0]
        none = O.linearise_fp64_multiview(dec, prm, [dict(view, pts=empty["pts"])], state[0], state[1], [state[2]], [dict(it["sets"], kept=O.NO_SETS["kept"])])
    assert none["K"] == 0 and none["N"] == 0 and none["Lr"] == 0 and none["Ls"] == 0 and not none["Dr"].any() and not none["Ds"].any()
    assert np.all(np.isfinite(none["H"])) and np.all(np.isfinite(none["dx"]))
    _parts_add_up(none)


@pytest.mark.parametrize("e", range(10))
def test_recorded_multiview_states_are_within_tau_of_the_pooled_fp64(oracle_decoder, e):
    g = golden("golden_multiview_cars3.npz")
    prm = O.GNParams.from_configs(json.loads(str(g["cfg_json"])))
    assert g["it_H"].shape[0] == 10
    views = MV.golden_views(g)
    it, itj, lin = X.linearise_at(oracle_decoder, prm, views, g["it_t_obj_cam"][e], g["it_code"][e], g["it_depths"][e])
    for v, (pv, pj) in enumerate(zip(it["views"], itj["views"])):
        rec = tuple(int(g["it_" + k][e][v]) for k in ("V", "K", "vsum", "ksum"))
        assert (pv["V"], pv["K"], pv["vsum"], pv["ksum"]) == rec
        assert (pj["V"], pj["K"], pj["vsum"], pj["ksum"]) == rec, "the jitter twin selects other sets"
    assert lin["K_views"] == [int(k) for k in g["it_K"][e]] and lin["V_views"] == [int(k) for k in g["it_V"][e]]
    assert lin["K"] == it["K"] and lin["N"] == it["M"]
    assert abs(lin["loss"] - it["loss"]) <= 1e-5 * abs(lin["loss"])
    _parts_add_up(lin)
    for who, s in (("composed fp32 oracle", it), ("its jitter twin", itj), ("reference", dict(H=g["it_H"][e], b=g["it_b"][e], dx=g["it_dx"][e]))):
        rec = M.scaled_errors(s, lin, prm.k4)
        print("iteration %d %-20s %s" % (e, who, M.flat(rec)))
        M.assert_within_tau(rec, "%s, iteration %d" % (who, e))


@pytest.mark.parametrize("name", list(X.CASES))
def test_the_gpu_cases_meet_their_conditions_on_the_composed_oracle(oracle_decoder, chairs32_decoder, name):
    case = X.CASES[name]()
    dec = _dec(case, oracle_decoder, chairs32_decoder)
    oprm = X.oracle_params(case)
    for i, obj in enumerate(case["objects"]):
        if obj.get("fails"):
            r = MV.reconstruct_object_multiview(dec, oprm, obj["t"], obj["views"], num_iterations=case["n_it"])
            assert not r["is_good"] and r["status"] == 1
            continue
        run = X.own_run(dec, oprm, obj, case["n_it"])
        assert len(run) == case["n_it"] and all(r is not None for r in run)
        for e, (it, itj, lin) in enumerate(run):
            assert X.same_sets(it, itj), "object %d iteration %d: a sample lies within the sdf round-off of a threshold; choose another seed" % (i, e)
            assert lin["K"] == it["K"] and lin["N"] == it["M"] and lin["K_views"] == [v["K"] for v in it["views"]]
            rec = M.scaled_errors(it, lin, oprm.k4)
            print("%s object %d iteration %d (V, K) %s: %s" % (name, i, e, X.view_vk(it), M.flat(rec)))
            M.assert_within_tau(rec, "%s object %d iteration %d" % (name, i, e))
        vk = [X.view_vk(it)[-1] for it, _, _ in run]          # the last view is the one a transition case is about
        if case.get("transition") == "join":
            assert vk[0][0] < 10 and run[0][0]["views"][1]["none"]
            first = min(e for e, (v, k) in enumerate(vk) if v >= 10 and k > 0)
            assert 0 < first < case["n_it"] - 1, "the iteration the view's rows first enter and one after it"
        elif case.get("transition") == "leave":
            assert vk[0][0] >= 10 and vk[0][1] > 0
            gone = [e for e, (v, k) in enumerate(vk) if k == 0]
            assert gone and all(vk[e][0] >= 10 for e in gone) and gone == list(range(gone[0], case["n_it"])) and len(gone) >= 2
            assert all(run[e][0]["K"] == run[e][0]["views"][0]["K"] for e in gone)
        elif case.get("transition") == "away":
            assert all(v < 10 and k == 0 for v, k in vk) and all(it["views"][1]["none"] for it, _, _ in run)
            assert all(it["M"] == sum(v["pts"].shape[0] for v in obj["views"]) for it, _, _ in run)


def _fault_states(dec):
    if not _FAULT_STATES:
        _FAULT_STATES.extend(X.fault_states(dec))
    return _FAULT_STATES


@pytest.mark.parametrize("k", range(len(X.FAULT_OBJECTS) * len(X.FAULT_ITERATIONS)))
def test_metric_rejects_member_view_faults(oracle_decoder, k):
    label, oprm, views, it, lin, prev_code = _fault_states(oracle_decoder)[k]
    base = M.scaled_errors(it, lin, oprm.k4)
    assert M.within_tau(base), M.flat(base)
    missed = []
    for what, sys_ in X.faults(oracle_decoder, oprm, views, it, prev_code).items():
        rec = M.scaled_errors(sys_, lin, oprm.k4)
        ok = M.within_tau(rec)
        print("%s: %-62s worst %.2e solve %.1e (%s)   max-norm check: %s" % (
            label, what, rec["worst"], rec["solve"], "ACCEPTED" if ok else "rejected", "passes" if X.max_norm_passes(sys_, it, oprm.k4) else "fails"))
        if ok and what in X.MUST_REJECT:
            missed.append((what, M.flat(rec)))
    assert not missed, missed
