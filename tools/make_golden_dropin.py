#!/usr/bin/env python3
"""tests/golden/golden_dropin.npz: what the UNMODIFIED reference's own loader helpers read from the KITTI-like files that
tests/test_dropin_delegation.py writes, and what its reference-only modules import from the modules this repository serves.

    python tools/make_golden_dropin.py

Needs a reference checkout (oracle/ref_shim.py: $DSP_REFERENCE_ROOT).  Records
  * calib_<key>: reconstruct/utils.py read_calib_file on the test's calib.txt (float64 arrays, one per key it returns);
  * velo:        reconstruct/utils.py load_velo_scan on the test's velodyne/000000.bin;
  * imports_json: {module: {"reconstruct.<mod>": [names]}} -- every `from reconstruct... import ...` of kitti_sequence.py,
    mono_sequence.py, detector2d.py and detector3d.py (read with ast; no source is copied).
Consumed by tests/test_dropin_delegation.py.
"""
import ast
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shim  # noqa: E402

GOLD = os.environ.get("DSP_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
REFERENCE_ONLY = ("kitti_sequence", "mono_sequence", "detector2d", "detector3d")


def reference_imports(pkg_dir):
    out = {}
    for mod in REFERENCE_ONLY:
        tree = ast.parse(open(os.path.join(pkg_dir, mod + ".py")).read())
        names = {}
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 0 and node.module and node.module.split(".")[0] == "reconstruct":
                names.setdefault(node.module, []).extend(a.name for a in node.names)
        out[mod] = {k: sorted(v) for k, v in sorted(names.items())}
    return out


def main():
    if not ref_shim.reference_available():
        raise SystemExit("no reference checkout (set DSP_REFERENCE_ROOT)")
    from test_dropin_delegation import write_kitti_dir
    ref_shim.install()
    pkg = os.path.join(ref_shim.REFERENCE_ROOT, "reconstruct")
    spec = importlib.util.spec_from_file_location("_ref_utils_for_golden", os.path.join(pkg, "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    with tempfile.TemporaryDirectory(prefix="dsp_dropin_") as d:
        write_kitti_dir(os.path.join(d, "k"))
        calib = ref.read_calib_file(os.path.join(d, "k", "calib.txt"))
        velo = ref.load_velo_scan(os.path.join(d, "k", "velodyne", "000000.bin"))
    rec = {"calib_" + k: np.asarray(v) for k, v in calib.items()}
    rec["velo"] = np.asarray(velo)
    rec["imports_json"] = np.array(json.dumps(reference_imports(pkg), sort_keys=True))
    os.makedirs(GOLD, exist_ok=True)
    np.savez(os.path.join(GOLD, "golden_dropin.npz"), **rec)
    print("wrote %s: %s" % (os.path.join(GOLD, "golden_dropin.npz"), sorted(rec)))


if __name__ == "__main__":
    main()
