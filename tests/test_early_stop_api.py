"""CPU: the interface of the per-object convergence rule -- its two C declarations and their ctypes prototypes, the Optimizer's optional
config keys (a reference config leaves the rule off), and the numpy statement of the rule (tests/early_stop_rule.py) at its edges."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import early_stop_rule as R
from conftest import ROOT
from dsp_slam_amd import _lib as L

INF = float("inf")


def test_declared_in_the_header_and_bound():
    src = open(os.path.join(ROOT, "include", "dsp_gn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+dsp_batch_convergence\s*\(\s*dsp_batch\s*\*\s*b\s*,\s*float\s+pose_tol\s*,\s*float\s+code_tol\s*,\s*int32_t\s+min_iterations\s*\)\s*;", code)
    assert re.search(r"int\s+dsp_batch_iterations_used\s*\(\s*dsp_batch\s*\*\s*b\s*,\s*int32_t\s*\*\s*out\s*\)\s*;", code)
    # a section of its own, not under the settings whose results are identical for every value
    assert src.index("results are identical, bit for bit, for every value") < src.index("---- convergence rule") < src.index("int dsp_batch_convergence")
    assert "#define DSP_OBJ_NAN 2" in src and "DSP_OBJ_DONE" not in src          # the public status values do not change
    sym = {n: (r, a) for n, r, a in L.SYMBOLS}
    assert sym["dsp_batch_convergence"] == (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int32])
    assert sym["dsp_batch_iterations_used"] == (C.c_int, [C.c_void_p, L.c_i32p])
    assert L.ABI_VERSION == 6
    lib = L.load()
    assert hasattr(lib, "dsp_batch_convergence") and hasattr(lib, "dsp_batch_iterations_used")


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


def _cfg(**edits):
    from reconstruct.utils import ForceKeyErrorDict

    def wrap(d):
        return ForceKeyErrorDict(**{k: wrap(v) if isinstance(v, dict) else v for k, v in d.items()})
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_kitti_optimizer.json")))
    cfg.setdefault("data_type", "KITTI")
    for path, v in edits.items():
        d = cfg
        keys = path.split("__")
        for k in keys[:-1]:
            d = d[k]
        d[keys[-1]] = v
    return wrap(cfg)


def test_optimizer_config_keys(mirror):
    from reconstruct.optimizer import Optimizer
    off = Optimizer(None, _cfg())                # the reference's config: no such keys, and its dict raises on a missing one
    assert off.convergence_joint is None and off.convergence_pose_only is None
    on = Optimizer(None, _cfg(optimizer__joint_optim__pose_tolerance=1e-3, optimizer__joint_optim__code_tolerance=2e-3,
                              optimizer__pose_only_optim__pose_tolerance=5e-4))
    assert on.convergence_joint == (1e-3, 2e-3) and on.convergence_pose_only == (5e-4, 0.0)
    half = Optimizer(None, _cfg(optimizer__joint_optim__pose_tolerance=1e-3))
    assert half.convergence_joint == (1e-3, INF) and half.convergence_pose_only is None

    class Eng(object):        # what the Optimizer hands to the engine: no `convergence` argument unless the config asks for one
        def __init__(self):
            self.kw = None

        def reconstruct_batch(self, prm, t, pts, rays, depth, codes, **kw):
            self.kw = kw
            n = len(pts)
            return np.zeros((n, 4, 4), np.float32), np.zeros((n, 64), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)

    class Dec(object):
        latent_size = 64
    for opt, want in ((off, None), (on, (1e-3, 2e-3))):
        opt.decoder = Dec()
        opt.decoder.engine = Eng()
        opt.reconstruct_objects([np.eye(4)], [np.zeros((3, 3))], [np.zeros((3, 3))], [np.zeros(3)])
        assert opt.decoder.engine.kw.get("convergence") == want and ("convergence" in opt.decoder.engine.kw) == (want is not None)


def test_rule_edges():
    dx = np.zeros((6, 71))
    for e in range(6):
        dx[e, :7] = 10.0 ** -(e + 1)         # pose steps 1e-1 .. 1e-6
        dx[e, 7:] = 10.0 ** -(e + 2)         # code steps 1e-2 .. 1e-7
    assert R.n_used(dx, 1.0, 0.0, 0.0) == 6 and R.n_used(dx, 1.0, 0.0, INF) == 6 and R.n_used(dx, 1.0, INF, 0.0) == 6      # tol 0 stops nothing
    assert R.n_used(dx, 1.0, INF, INF) == 1 and R.n_used(dx, 1.0, INF, INF, min_iterations=4) == 4
    assert R.n_used(dx, 1.0, INF, INF, min_iterations=7) == 6
    assert R.n_used(dx, 1.0, 3e-3, INF) == 3 and R.n_used(dx, 1.0, INF, 3e-3) == 2 and R.n_used(dx, 1.0, 3e-3, 3e-6) == 5
    assert R.n_used(dx, 1.0, 1e-3, INF) == 4           # strict: a step equal to the tolerance does not pass
    assert R.n_used(dx, 0.5, 3e-3, INF) == 3 and R.n_used(dx, 0.5, 4e-4, INF) == 4 and R.n_used(dx, 0.01, 3e-3, INF) == 1     # the step is lr dx
    bad = dx.copy()
    bad[2, 3] = np.nan                                  # a NaN step never passes, not even against inf
    assert R.n_used(bad, 1.0, INF, INF, min_iterations=3) == 4 and R.n_used(bad, 1.0, 3e-3, INF) == 4
    bad = dx.copy()
    bad[:, 40] = np.nan
    assert R.n_used(bad, 1.0, INF, INF) == 6
    p6 = dx[:, :6]
    assert R.n_used(p6, 0.01, 3e-3, 0.0, n_pose=6, pose_only=True) == 3           # pose-only: 6 entries, dx itself, code_tol ignored
    assert R.n_used(p6, 1.0, 0.0, INF, n_pose=6, pose_only=True) == 6
