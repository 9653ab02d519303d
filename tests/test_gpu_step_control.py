"""GPU: Levenberg-Marquardt step control (dsp_batch_step_control / dsp_batch_step_log, include/dsp_gn.h; the rule: csrc/step_rule.h).

The batch is the six-object batch of tests/test_gpu_early_stop.py: three cold objects (160 surface points + 200 rays) and the same three
warm-started from their own 10-iteration results.  Comparisons are EXACT (bit for bit) unless a bound is stated: objects are independent,
an iteration restarted from its traced state reproduces itself, and the rule is a handful of fp64 comparisons and products, so every
consequence of an acceptance or a rejection can be reproduced by a second run.  The input conditions (which objects reject, and when)
are asserted, not assumed; tests/test_step_control_host.py shows them on the CPU oracle.
"""
import numpy as np
import pytest

import step_control_ref as S
import test_gpu_early_stop as ES
from dsp_slam_amd import _lib as L, engine as E

pytestmark = pytest.mark.gpu
INF = float("inf")
OFF = (0.0, 0.0, 0.0, 0.0, 0.0)
DEFAULTS = (0.0, 10.0, 0.1, 1.0, INF)
N = 14
COLD = [0, 1, 2]


@pytest.fixture(scope="module")
def eng(oracle_decoder):
    e = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)
    yield e
    e.close()


def _traces(b, n_it):
    return [b.trace(e) for e in range(n_it)]


def _run(eng, objs, prm, n_it, step=None, trace=False, start=None, before_run=None):
    """One run of a fresh batch -> dict(rows, used, log (or None), tr (or None))."""
    b = ES._batch(eng, objs, prm, trace=trace)
    try:
        b.set_iterations(n_it)
        if step is not None:
            b.set_step_control(*step)
        if start is not None:
            b.set_start_state(*start)
        if before_run is not None:
            before_run(b)
        b.run()
        out = dict(rows=b.results(), used=b.iterations_used(), log=b.step_log() if step is not None else None, tr=_traces(b, n_it) if trace else None)
        if before_run is not None:
            out["batch_extras"] = before_run(b, after=True)
        return out
    finally:
        b.close()


class Setup(object):
    """The six objects and the traced step-controlled run of N iterations every test reads (made once)."""

    def __init__(self, eng):
        self.prm = E.gn_params(num_iterations=10, lr=1.0)
        cold = ES._cold()
        self.objs = cold + ES._warm_from(eng, cold, self.prm)
        self.sc = _run(eng, self.objs, self.prm, N, step=DEFAULTS, trace=True)
        lg = self.sc["log"]
        print("decisions\n", lg["decision"].T, "\ncosts\n", np.array2string(lg["cost"].T, precision=5), "\nlambdas\n", lg["lambda"].T,
              "\nreturned loss", self.sc["rows"][2])
        assert (self.sc["rows"][3] == 0).all()

    def accepted_source(self, i, e):
        """The last accepted iteration <= e of object i."""
        d = self.sc["log"]["decision"][:, i]
        return max(a for a in range(e + 1) if d[a] == S.ACCEPTED)


@pytest.fixture(scope="module")
def setup(eng):
    return Setup(eng)


def _trace_equal(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# 1 ----------------------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(eng, setup):
    """A batch that had step control set and then switched off returns the rows, traces and iteration counts of one that never had it."""
    never = _run(eng, setup.objs, setup.prm, 10, trace=True)
    b = ES._batch(eng, setup.objs, setup.prm, trace=True)
    b.set_step_control(*DEFAULTS)
    b.set_step_control(*OFF)
    b.run()
    rows, used, tr = b.results(), b.iterations_used(), _traces(b, 10)
    with pytest.raises(L.DspError, match=r"\(-4\)"):
        b.step_log()
    b.close()
    assert ES._same(rows, never["rows"]) and np.array_equal(used, never["used"]) and (used == 10).all()
    assert all(_trace_equal(x, y) for x, y in zip(tr, never["tr"]))


# 2 ----------------------------------------------------------------------------------------------------------------------------------------
def test_one_iteration_returns_the_initial_state(eng, setup):
    one = _run(eng, setup.objs, setup.prm, 1, step=DEFAULTS, trace=True)
    plain = _run(eng, setup.objs, setup.prm, 1)
    t, code, loss, status = one["rows"]
    assert (status == 0).all() and (one["used"] == 1).all()
    assert np.array_equal(loss, plain["rows"][2])                                   # the loss AT the initial state
    assert (one["log"]["decision"] == S.ACCEPTED).all() and np.array_equal(one["log"]["cost"][0], loss.astype(np.float64))
    tr = one["tr"][0]
    assert not tr["dx"].any()                                                       # no step was applied
    for i, o in enumerate(setup.objs):
        assert np.array_equal(code[i], o.get("code0", np.zeros(64, np.float32))[:code.shape[1]])
        assert np.array_equal(code[i], tr["code"][i][:code.shape[1]])
        t_co = np.linalg.inv(tr["t_obj_cam"][i].astype(np.float64))
        assert np.abs(t_co - t[i]).max() <= 1e-5 * np.abs(t[i]).max()
        assert np.abs(np.asarray(o["t_cam_obj_init"], np.float64) - t[i]).max() <= 1e-5 * np.abs(t[i]).max()


# 3 ----------------------------------------------------------------------------------------------------------------------------------------
def test_all_accepted_is_the_plain_iteration(eng, setup):
    """lambda0 = 0, five iterations: with every trial accepted the run is four plain updates plus one evaluation."""
    sc = _run(eng, setup.objs, setup.prm, 5, step=DEFAULTS)
    assert (sc["log"]["decision"][:, COLD] == S.ACCEPTED).all(), sc["log"]["decision"].T       # input condition (the oracle: wide margins)
    assert not sc["log"]["lambda"][:, COLD].any()
    p4, p5 = _run(eng, setup.objs, setup.prm, 4), _run(eng, setup.objs, setup.prm, 5)
    assert np.array_equal(sc["rows"][0][COLD], p4["rows"][0][COLD]) and np.array_equal(sc["rows"][1][COLD], p4["rows"][1][COLD])
    assert np.array_equal(sc["rows"][2][COLD], p5["rows"][2][COLD])
    assert (sc["rows"][3] == 0).all() and (sc["used"] == 5).all()


# 4 ----------------------------------------------------------------------------------------------------------------------------------------
def test_log_replay(eng, setup):
    lg, tr = setup.sc["log"], setup.sc["tr"]
    dec, cost, lam = lg["decision"], lg["cost"], lg["lambda"]
    assert (dec != S.NOT_EVALUATED).all() and (setup.sc["used"] == N).all()
    lr = np.float32(setup.prm.lr)
    n_checked = 0
    for i in range(len(setup.objs)):
        want_dec, want_lam = S.rule(cost[:, i], *DEFAULTS)
        assert np.array_equal(dec[:, i], want_dec) and np.array_equal(lam[:, i], want_lam), i
        acc = cost[dec[:, i] == S.ACCEPTED, i]
        assert np.all(acc[1:] < acc[:-1]), (i, acc)
        rej = np.flatnonzero(dec[:, i] == S.REJECTED)
        if i in COLD:                                                               # input condition
            assert rej.size and (dec[rej[0]:, i] == S.ACCEPTED).any(), (i, dec[:, i])
        a_last = setup.accepted_source(i, N - 1)
        assert setup.sc["rows"][2][i] == np.float32(cost[a_last, i]) and float(setup.sc["rows"][2][i]) == cost[a_last, i]
        for e in range(N):
            a = setup.accepted_source(i, e)
            dx = tr[e]["dx"][i]
            if e == N - 1:
                assert not dx.any()
                continue
            h64 = tr[a]["H"][i].astype(np.float64)
            b64 = tr[a]["b"][i].astype(np.float64)
            hl = h64 + lam[e, i] * np.eye(71)
            dx64 = np.linalg.solve(hl, b64)
            # the bound of test_solve_against_float64_lapack for the traced (float32-rounded) system
            bound = np.abs(np.linalg.inv(hl)) @ (6e-8 * (np.abs(h64) @ np.abs(dx64) + np.abs(b64))) + 2e-7 * np.abs(dx64).max()
            err = np.abs(dx - dx64)
            assert np.all(err <= 4 * bound), (i, e, float((err / bound).max()))
            # the state iteration e + 1 starts from is the step applied to the ACCEPTED state (a rejected trial is discarded)
            want_code = (tr[a]["code"][i] + lr * dx[7:]).astype(np.float32)
            assert np.array_equal(tr[e + 1]["code"][i], want_code), (i, e)
            want_t = eng.debug_lie(3, np.concatenate([tr[a]["t_obj_cam"][i].reshape(-1), lr * dx[:7]])).reshape(4, 4)
            assert np.array_equal(tr[e + 1]["t_obj_cam"][i], want_t), (i, e)
            if a != e:
                from_trial = eng.debug_lie(3, np.concatenate([tr[e]["t_obj_cam"][i].reshape(-1), lr * dx[:7]])).reshape(4, 4)
                assert not np.array_equal(tr[e + 1]["t_obj_cam"][i], from_trial)
                n_checked += 1
    assert n_checked >= 3


# 5 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", COLD)
def test_a_resolve_is_a_fresh_first_step(eng, setup, i):
    dec, lam, tr = setup.sc["log"]["decision"], setup.sc["log"]["lambda"], setup.sc["tr"]
    e = next(e for e in range(N - 1) if dec[e, i] == S.REJECTED)
    a = setup.accepted_source(i, e)
    new = _run(eng, [setup.objs[i]], setup.prm, 2, step=(lam[e, i],) + DEFAULTS[1:], trace=True,
               start=([tr[a]["t_obj_cam"][i]], [tr[a]["code"][i]]))
    assert np.array_equal(new["tr"][0]["t_obj_cam"][0], tr[a]["t_obj_cam"][i])
    assert np.array_equal(new["tr"][1]["t_obj_cam"][0], tr[e + 1]["t_obj_cam"][i])
    assert np.array_equal(new["tr"][1]["code"][0], tr[e + 1]["code"][i])


# 6 ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_loss_belongs_to_the_returned_state(eng, setup):
    tr = setup.sc["tr"]
    last = [setup.accepted_source(i, N - 1) for i in range(len(setup.objs))]
    start = ([tr[a]["t_obj_cam"][i] for i, a in enumerate(last)], [tr[a]["code"][i] for i, a in enumerate(last)])
    plain = _run(eng, setup.objs, setup.prm, 1, start=start)
    one = _run(eng, setup.objs, setup.prm, 1, step=DEFAULTS, start=start)
    t, code, loss, _ = setup.sc["rows"]
    assert np.array_equal(loss, plain["rows"][2])
    for i, a in enumerate(last):
        assert np.array_equal(code[i], tr[a]["code"][i][:code.shape[1]])
    assert np.array_equal(t, one["rows"][0]) and np.array_equal(code, one["rows"][1]) and np.array_equal(loss, one["rows"][2])


# 7 ----------------------------------------------------------------------------------------------------------------------------------------
def test_convergence_rule(eng, setup):
    lr = 1.0
    tr = setup.sc["tr"]
    dx = np.stack([t["dx"] for t in tr[:N - 1]]).astype(np.float64)                 # the last row holds no solved step (zeros)
    sp, sc = np.abs(lr * dx[:, :, :7]).max(-1), np.abs(lr * dx[:, :, 7:]).max(-1)
    print("pose steps\n", sp.T, "\ncode steps\n", sc.T)

    def predict(tp, tc):
        out = []
        for i in range(dx.shape[1]):
            n = ES.R.n_used(dx[:, i], lr, tp, tc)
            hit = bool(np.all(np.abs(lr * dx[n - 1, i, :7]) < tp) and np.all(np.abs(lr * dx[n - 1, i, 7:]) < tc))
            out.append(n if hit else N)
        return np.array(out, np.int32)

    def cands(s):
        out = [float(np.sqrt(s[e, i] * s[e + 1, i])) for i in range(s.shape[1]) for e in range(s.shape[0] - 1)]
        return [t for t in out if t > 0 and ES._far(s, t)]
    tol = next(((tp, tc) for tp in cands(sp) for tc in cands(sc) if predict(tp, tc)[COLD].min() < N and len(set(predict(tp, tc).tolist())) >= 2), None)
    assert tol is not None, "no tolerance pair freezes a cold object before iteration %d" % N       # input condition
    want = predict(*tol)

    def with_rule(b, after=False):
        if not after:
            b.set_convergence(tol[0], tol[1], 1)
    got = _run(eng, setup.objs, setup.prm, N, step=DEFAULTS, before_run=with_rule)
    used, dec = got["used"], got["log"]["decision"]
    print("tolerances", tol, "predicted", want, "used", used)
    assert np.array_equal(used, want) and (got["rows"][3] == 0).all()
    assert np.array_equal((dec != S.NOT_EVALUATED).sum(0).astype(np.int32), used)
    for i, n in enumerate(used):
        assert (dec[:n, i] != S.NOT_EVALUATED).all() and (dec[n:, i] == S.NOT_EVALUATED).all()
        assert np.array_equal(dec[:n, i], setup.sc["log"]["decision"][:n, i]) and np.array_equal(got["log"]["cost"][:n, i], setup.sc["log"]["cost"][:n, i])
        a = setup.accepted_source(i, n - 1)                                         # frozen at its last accepted state
        assert np.array_equal(got["rows"][1][i], tr[a]["code"][i][:got["rows"][1].shape[1]])
        assert float(got["rows"][2][i]) == setup.sc["log"]["cost"][a, i]
    for n in sorted(set(used.tolist())):                                            # ... which is what a run of n iterations returns
        fixed = _run(eng, setup.objs, setup.prm, n, step=DEFAULTS)
        assert ES._same(got["rows"], fixed["rows"], used == n), n


# 8 ----------------------------------------------------------------------------------------------------------------------------------------
def test_posterior(eng, setup):
    def with_posterior(b, after=False):
        if after:
            return b.posterior()
        b.set_posterior(1, "mean")
    got = _run(eng, setup.objs, setup.prm, N, step=DEFAULTS, before_run=with_posterior)
    assert ES._same(got["rows"], setup.sc["rows"]) and np.array_equal(got["used"], setup.sc["used"])
    assert np.array_equal(got["log"]["decision"], setup.sc["log"]["decision"]) and np.array_equal(got["log"]["cost"], setup.sc["log"]["cost"])
    rec = got["batch_extras"]
    assert (rec["status"] == L.POSTERIOR_OK).all()
    assert np.array_equal(rec["loss"], got["rows"][2])                              # the pass linearises at the returned state


# 9 ----------------------------------------------------------------------------------------------------------------------------------------
def test_prior(eng, setup):
    def level2(b, after=False):
        if after:
            return b.posterior()
        b.set_posterior(2, "mean")
    rec = _run(eng, setup.objs, setup.prm, 10, before_run=level2)["batch_extras"]
    assert (rec["status"] == L.POSTERIOR_OK).all()

    def with_prior(b, after=False):
        if after:
            return b.prior_residual()
        b.set_prior(rec["t_obj_cam"], rec["code"], rec["Lambda"])
    got = _run(eng, setup.objs, setup.prm, N, step=DEFAULTS, before_run=with_prior)
    assert (got["rows"][3] == 0).all()
    dec, cost = got["log"]["decision"], got["log"]["cost"]
    chi2 = got["batch_extras"]["chi2"]
    print("prior: decisions\n", dec.T, "\nchi2", chi2)
    for i in range(len(setup.objs)):
        a = max(e for e in range(N) if dec[e, i] == S.ACCEPTED)
        assert cost[a, i] == float(got["rows"][2][i]) + chi2[i], (i, cost[a, i], got["rows"][2][i], chi2[i])
    assert np.all(chi2 > 0)


# 10 ---------------------------------------------------------------------------------------------------------------------------------------
def test_learning_rate_of_four(eng, setup):
    prm = E.gn_params(num_iterations=6, lr=4.0)
    cold = setup.objs[:3]
    plain = _run(eng, cold, prm, 6)
    assert (plain["rows"][3] != 0).all(), plain["rows"][3]                          # input condition, on the device
    sc = _run(eng, cold, prm, 6, step=DEFAULTS)
    print("lr 4: decisions\n", sc["log"]["decision"].T, "\ncosts\n", sc["log"]["cost"].T)
    assert (sc["rows"][3] == L.OBJ_GOOD).all()
    assert np.all(sc["rows"][2].astype(np.float64) < sc["log"]["cost"][0])


# 11 ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng, setup):
    from conftest import golden
    g = golden("golden_pose_only.npz")
    pb = eng.pose_batch(E.gn_params(), [g["t_co_se3"]], [float(g["scale"])], [g["pts"][:200]], [g["code"]])
    with pytest.raises(L.DspError, match=r"\(-1\)"):
        pb.set_step_control(*DEFAULTS)
    pb.set_step_control(*OFF)
    pb.close()
    o = setup.objs[0]
    mv = eng.multiview_batch(setup.prm, [o["t_cam_obj_init"]], [ES._views(o)], [np.zeros(64, np.float32)])
    with pytest.raises(L.DspError, match=r"\(-1\)"):
        mv.set_step_control(*DEFAULTS)
    mv.close()
    b = ES._batch(eng, setup.objs[:1], setup.prm)
    b.set_step_control(*DEFAULTS)
    with pytest.raises(L.DspError, match=r"\(-4\)"):
        b.step_log()                                                                # before a run
    with pytest.raises(L.DspError, match=r"\(-1\)"):
        b.set_step_control(0.0, 1.0, 0.1, 1.0, INF)                                 # refused: the previous setting stays
    b.set_iterations(3)
    b.run()
    assert b.step_log()["decision"].shape == (3, 1) and (b.step_log()["decision"] != 0).all()
    b.close()


# 12 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(6))
def test_ragged_batch_equals_single_runs(eng, setup, i):
    one = _run(eng, [setup.objs[i]], setup.prm, N, step=DEFAULTS)
    assert ES._same(one["rows"], tuple(x[i:i + 1] for x in setup.sc["rows"]))
    for k in ("decision", "cost", "lambda"):
        assert np.array_equal(one["log"][k][:, 0], setup.sc["log"][k][:, i]), k


# the one-call form ------------------------------------------------------------------------------------------------------------------------
def test_engine_one_call_form(eng, setup):
    args = ([o["t_cam_obj_init"] for o in setup.objs], [o["pts"] for o in setup.objs], [o["rays"] for o in setup.objs], [o["depth"] for o in setup.objs],
            [o.get("code0", np.zeros(64, np.float32)) for o in setup.objs])
    want = _run(eng, setup.objs, setup.prm, 10, step=DEFAULTS)["rows"]
    assert ES._same(eng.reconstruct_batch(setup.prm, *args, step_control=True), want)
    assert ES._same(eng.reconstruct_batch(setup.prm, *args, step_control=DEFAULTS), want)
    assert ES._same(eng.reconstruct_batch(setup.prm, *args, step_control=dict(up=10.0)), want)
    assert not ES._same(eng.reconstruct_batch(setup.prm, *args), want)


# the partial re-run after a prepass-guard trip; the low-precision compute mode ------------------------------------------------------------
def test_guard_rerun(oracle_decoder, setup):
    """A forced bf16 margin of 2e-5 trips the guard (tests/test_gpu_prepass.py): the tripped objects run again with the prepass off and the
    rule started afresh, the others keep their rows, so rows, counts and the log are those of the prepass-off run."""
    own = E.Engine(oracle_decoder.layers, oracle_decoder.latent_in, oracle_decoder.code_len, device=0)      # (a trip is recorded on the handle)
    out = {}
    for name, mode, delta in (("off", L.PREPASS_OFF, -1.0), ("trip", L.PREPASS_BF16, 2e-5)):
        def with_prepass(b, after=False, mode=mode, delta=delta):
            if after:
                return b.stats()
            b.set_prepass(mode, delta)
        out[name] = _run(own, setup.objs, setup.prm, N, step=DEFAULTS, before_run=with_prepass)
    own.close()
    st = out["trip"]["batch_extras"]
    assert st["prepass_guard_rerun"] == 1 and st["prepass_guard_trips"] > 0
    assert ES._same(out["trip"]["rows"], out["off"]["rows"]) and np.array_equal(out["trip"]["used"], out["off"]["used"])
    for k in ("decision", "cost", "lambda"):
        assert np.array_equal(out["trip"]["log"][k], out["off"]["log"][k]), k
    assert ES._same(out["off"]["rows"], setup.sc["rows"])


def test_low_precision_compute_mode(eng, setup):
    def f16(b, after=False):
        if not after:
            b.set_compute(L.COMPUTE_F16)
    got = _run(eng, setup.objs, setup.prm, N, step=DEFAULTS, before_run=f16)
    dec, cost, lam = got["log"]["decision"], got["log"]["cost"], got["log"]["lambda"]
    assert (got["rows"][3] == 0).all() and (dec != S.NOT_EVALUATED).all()
    for i in range(len(setup.objs)):
        want_dec, want_lam = S.rule(cost[:, i], *DEFAULTS)
        assert np.array_equal(dec[:, i], want_dec) and np.array_equal(lam[:, i], want_lam), i
        a = max(e for e in range(N) if dec[e, i] == S.ACCEPTED)
        assert float(got["rows"][2][i]) == cost[a, i] and cost[a, i] < cost[0, i]
