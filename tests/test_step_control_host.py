"""CPU: Levenberg-Marquardt step control (dsp_batch_step_control, include/dsp_gn.h; the rule: dsp_slam_amd/csrc/step_rule.h).

1. dsp_debug_step_rule -- the very function k_solve<.., STEP = true> runs, compiled for the host -- against the numpy restatement of
   tests/step_control_ref.py: decisions and lambdas equal EXACTLY (the rule is comparisons, products by the factors, min and max).
2. Every argument dsp_batch_step_control refuses is refused (DSP_E_ARG).
3. The rule composed from unmodified oracle pieces (step_control_ref.run) on the three objects of the GPU tests: what the feature is for,
   and the input conditions the GPU tests rely on.
"""
import ctypes as C

import numpy as np
import pytest

import step_control_ref as S
from dsp_slam_amd import _lib as L, synth

INF = float("inf")
NAN = float("nan")
OK, E_ARG = 0, -1          # DSP_OK, DSP_E_ARG (include/dsp_gn.h)
DEFAULTS = (0.0, 10.0, 0.1, 1.0, INF)


def _device_rule(cost, lambda0, up, down, lambda_min, lambda_max):
    cost = np.ascontiguousarray(cost, np.float64)
    dec, lam = np.full(cost.shape[0], -1, np.int32), np.full(cost.shape[0], NAN)
    rc = L.load().dsp_debug_step_rule(cost.shape[0], L.ptr(cost, L.c_f64p), lambda0, up, down, lambda_min, lambda_max, L.ptr(dec, L.c_i32p),
                                      L.ptr(lam, L.c_f64p))
    assert rc == OK, rc
    return dec, lam


SEQUENCES = {
    "accept_run": [5.0, 4.0, 3.0, 2.5, 2.0, 1.0],
    "reject_run": [1.0, 2.0, 3.0, 1.5, 1.0000001, 7.0],
    "mixed": [0.304, 0.129, 0.083, 0.050, 0.041, 0.028, 0.018, 0.0103, 0.042, 0.081, 0.02, 0.0102, 0.0101, 0.0105],
    "ties": [1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25],
    "nan": [1.0, NAN, 0.5, NAN, NAN, 0.4],
    "nan_first": [NAN, 1.0, 0.5],
    "one": [3.0],
    "empty": [],
}
SETTINGS = {
    "defaults": DEFAULTS,
    "lambda0": (0.5, 10.0, 0.1, 1.0, INF),
    "small_factors": (0.0, 2.0, 0.5, 0.1, INF),
    "capped": (0.0, 10.0, 0.1, 1.0, 250.0),
    "cap_is_min": (3.0, 10.0, 1.0, 2.0, 2.0),
}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_rule_equals_its_restatement(seq, setting):
    want = S.rule(SEQUENCES[seq], *SETTINGS[setting])
    got = _device_rule(SEQUENCES[seq], *SETTINGS[setting])
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])      # exactly: no tolerance


def test_rule_by_hand():
    """The fixtures the restatement itself is checked on, written out."""
    dec, lam = _device_rule([4.0, 3.0, 3.0, 2.0, NAN, 5.0, 1.0], *DEFAULTS)
    # accept (lambda0 = 0), accept (0 * 0.1 = 0), tie -> reject (max(0, 1) * 10), accept (10 * 0.1), NaN -> reject, reject, accept
    assert dec.tolist() == [1, 1, 2, 1, 2, 2, 1]
    assert lam.tolist() == [0.0, 0.0, 10.0, 10.0 * 0.1, (10.0 * 0.1) * 10.0, ((10.0 * 0.1) * 10.0) * 10.0, (((10.0 * 0.1) * 10.0) * 10.0) * 0.1]
    # lambda0 = 0 stays 0 under acceptance and becomes lambda_min * up on the first rejection
    dec, lam = _device_rule([5.0, 4.0, 3.0, 2.0, 9.0], 0.0, 4.0, 0.5, 0.25, INF)
    assert dec.tolist() == [1, 1, 1, 1, 2] and lam.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    # the cap
    dec, lam = _device_rule([1.0, 2.0, 2.0, 2.0, 2.0], 0.0, 10.0, 0.1, 1.0, 250.0)
    assert dec.tolist() == [1, 2, 2, 2, 2] and lam.tolist() == [0.0, 10.0, 100.0, 250.0, 250.0]
    # an acceptance compares with the ACCEPTED cost, not with the previous trial's
    dec, _ = _device_rule([1.0, 3.0, 2.0, 0.9], *DEFAULTS)
    assert dec.tolist() == [1, 2, 2, 1]


REFUSED = {
    "off_is_no_rule": (0.0, 0.0, 0.0, 0.0, 0.0),
    "nan_lambda0": (NAN, 10.0, 0.1, 1.0, INF),
    "inf_lambda0": (INF, 10.0, 0.1, 1.0, INF),
    "nan_up": (0.0, NAN, 0.1, 1.0, INF),
    "inf_up": (0.0, INF, 0.1, 1.0, INF),
    "nan_down": (0.0, 10.0, NAN, 1.0, INF),
    "nan_lambda_min": (0.0, 10.0, 0.1, NAN, INF),
    "inf_lambda_min": (0.0, 10.0, 0.1, INF, INF),
    "nan_lambda_max": (0.0, 10.0, 0.1, 1.0, NAN),
    "minus_inf_lambda_max": (0.0, 10.0, 0.1, 1.0, -INF),
    "negative_lambda0": (-1e-9, 10.0, 0.1, 1.0, INF),
    "up_is_one": (0.0, 1.0, 0.1, 1.0, INF),
    "up_below_one": (0.0, 0.5, 0.1, 1.0, INF),
    "down_zero": (0.0, 10.0, 0.0, 1.0, INF),
    "down_negative": (0.0, 10.0, -0.1, 1.0, INF),
    "down_above_one": (0.0, 10.0, 1.0000001, 1.0, INF),
    "lambda_min_zero": (0.0, 10.0, 0.1, 0.0, INF),
    "lambda_min_negative": (0.0, 10.0, 0.1, -1.0, INF),
    "max_below_min": (0.0, 10.0, 0.1, 1.0, 0.5),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_arguments(name):
    cost = np.array([1.0, 2.0])
    rc = L.load().dsp_debug_step_rule(2, L.ptr(cost, L.c_f64p), *REFUSED[name], None, None)
    assert rc == E_ARG, (name, rc)


def test_accepted_edge_arguments():
    """The edges of the accepted ranges: down = 1, lambda_max = lambda_min, lambda_max = +inf, lambda0 = 0; outputs may be NULL."""
    cost = np.array([1.0, 2.0])
    lib = L.load()
    for args in ((0.0, 1.0000001, 1.0, 1e-300, 1e-300), (0.0, 10.0, 0.1, 1.0, INF), (7.0, 2.0, 0.5, 3.0, 3.0)):
        assert lib.dsp_debug_step_rule(2, L.ptr(cost, L.c_f64p), *args, None, None) == OK, args
    assert lib.dsp_debug_step_rule(-1, L.ptr(cost, L.c_f64p), *DEFAULTS, None, None) == E_ARG
    assert lib.dsp_debug_step_rule(2, None, *DEFAULTS, None, None) == E_ARG


def test_bindings_and_python_surface():
    from dsp_slam_amd import engine as E
    bound = {n: (r, a) for n, r, a in L.SYMBOLS}
    assert bound["dsp_batch_step_control"][1] == [C.c_void_p] + [C.c_double] * 5
    assert len(bound["dsp_batch_step_log"][1]) == 4 and len(bound["dsp_debug_step_rule"][1]) == 9
    assert callable(E.Batch.set_step_control) and callable(E.Batch.step_log)
    assert E._step_control_args(True) == {}
    assert E._step_control_args((0.0, 10.0, 0.1, 1.0, INF)) == dict(lambda0=0.0, up=10.0, down=0.1, lambda_min=1.0, lambda_max=INF)
    assert E._step_control_args(dict(up=2.0)) == dict(up=2.0)


# ---- the rule composed from unmodified oracle pieces ------------------------------------------------------------------------------------
def _objects():
    return [synth.make_object(300, n_surface=160, n_background=40), synth.make_object(301, n_surface=160, n_background=40),
            synth.make_object(302, n_surface=160, n_background=40, t_noise=0.6, yaw_noise_deg=15.0)]


@pytest.fixture(scope="module")
def composed(oracle_decoder):
    from oracle import dsp_oracle as O
    out = []
    for o in _objects():
        p = O.GNParams(num_iterations=10)
        plain = O.reconstruct_object(oracle_decoder, p, o["t_cam_obj_init"], o["pts"], o["rays"], o["depth"])
        p4 = O.GNParams(num_iterations=6, lr=4.0)
        plain4 = O.reconstruct_object(oracle_decoder, p4, o["t_cam_obj_init"], o["pts"], o["rays"], o["depth"])
        out.append(dict(plain=plain, sc14=S.run(oracle_decoder, p, o, 14), plain4=plain4, sc4=S.run(oracle_decoder, p4, o, 6)))
        print("plain loss %.5f  step control (14): loss %.5f decisions %s  lr 4: plain good %s, step control good %s loss %.5f" % (
            plain["loss"], out[-1]["sc14"]["loss"], out[-1]["sc14"]["decision"], plain4["is_good"], out[-1]["sc4"]["is_good"], out[-1]["sc4"]["loss"]))
    return out


@pytest.mark.parametrize("i", range(3))
def test_composed_oracle_accepted_costs_decrease(composed, i):
    r = composed[i]["sc14"]
    assert r["is_good"] and len(r["decision"]) == 14
    acc = [c for c, d in zip(r["cost"], r["decision"]) if d == S.ACCEPTED]
    assert len(acc) >= 2 and all(b < a for a, b in zip(acc, acc[1:])), acc
    assert r["loss"] == acc[-1]
    # the input conditions of the GPU tests: no rejection in the first five iterations, a rejection with an acceptance after it later
    assert all(d == S.ACCEPTED for d in r["decision"][:5])
    rej = [e for e, d in enumerate(r["decision"]) if d == S.REJECTED]
    assert rej and any(d == S.ACCEPTED for d in r["decision"][rej[0]:])
    dec, lam = S.rule(r["cost"])
    assert dec.tolist() == r["decision"] and lam.tolist() == r["lam"]


@pytest.mark.parametrize("i", range(3))
def test_composed_oracle_returns_a_lower_loss_than_the_plain_run(composed, i):
    assert composed[i]["plain"]["is_good"]
    assert composed[i]["sc14"]["loss"] < composed[i]["plain"]["loss"]


@pytest.mark.parametrize("i", range(3))
def test_composed_oracle_survives_a_learning_rate_of_four(composed, i):
    assert composed[i]["plain4"]["is_good"] is False
    r = composed[i]["sc4"]
    assert r["is_good"] and r["loss"] < r["cost"][0]


@pytest.fixture
def mirror():
    """The package directory on sys.path, as the drop-in layout has it (reconstruct.*, deep_sdf.* importable by those names)."""
    import os
    import sys
    from conftest import ROOT
    pkg = os.path.join(ROOT, "dsp_slam_amd")
    sys.path.insert(0, pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]
    yield
    sys.path.remove(pkg)
    for m in [k for k in sys.modules if k.split(".")[0] in ("reconstruct", "deep_sdf")]:
        del sys.modules[m]


def test_optimizer_config_key(mirror):
    """joint_optim.step_control: absent / false = off; true, a dict or a five-item list go to Engine.reconstruct_batch(step_control=...)."""
    import copy
    import json
    import os
    from conftest import ROOT
    from reconstruct.optimizer import Optimizer
    from reconstruct.utils import ForceKeyErrorDict
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    base.setdefault("data_type", "KITTI")

    def optimizer(value=None):
        cfg = copy.deepcopy(base)
        if value is not None:
            cfg["optimizer"]["joint_optim"]["step_control"] = value
        return Optimizer(None, ForceKeyErrorDict(cfg))
    assert optimizer().step_control_joint is None and optimizer(False).step_control_joint is None
    assert optimizer(True).step_control_joint is True
    assert optimizer({"up": 4, "lambda_min": 0.5}).step_control_joint == dict(up=4.0, lambda_min=0.5)
    assert optimizer([0, 10, 0.1, 1, 1e6]).step_control_joint == (0.0, 10.0, 0.1, 1.0, 1e6)
    for bad in ({"upp": 2}, [0, 10, 0.1]):
        with pytest.raises(ValueError):
            optimizer(bad)

    class FakeEngine(object):
        def reconstruct_batch(self, prm, t, pts, rays, depth, codes=None, **kw):
            self.kw = kw
            n = len(pts)
            return np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), np.zeros((n, 64), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    opt = optimizer({"up": 4})
    opt.verbose = False
    eng = FakeEngine()
    opt.decoder = type("D", (), {"engine": eng})()
    pts, rays, depth = np.zeros((4, 3), np.float32), np.zeros((6, 3), np.float32), np.zeros(4, np.float32)
    assert opt.reconstruct_object(np.eye(4, dtype=np.float32), pts, rays, depth).is_good
    assert eng.kw["step_control"] == dict(up=4.0)
    opt = optimizer()
    opt.verbose = False
    opt.decoder = type("D", (), {"engine": eng})()
    opt.reconstruct_object(np.eye(4, dtype=np.float32), pts, rays, depth)
    assert "step_control" not in eng.kw
