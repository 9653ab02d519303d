#!/usr/bin/env python3
"""The `depth_envelope` records that tests/test_gpu_depth_envelope.py writes through tests/conftest.py:parity_log (a directory of *.jsonl
files, one per pytest session) -> the tables of profiles/depth_envelope.md, latest record per case:
   python tools/make_depth_envelope_report.py PARITY_DIR >> profiles/depth_envelope.md"""
import json
import os
import sys


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = sys.argv[1]
    recs = sorted((json.loads(ln) for f in sorted(os.listdir(path)) if f.endswith(".jsonl") for ln in open(os.path.join(path, f)) if ln.strip()),
                  key=lambda r: r.get("_t", 0.0))
    last = {}
    for r in recs:
        if str(r.get("kind", "")).startswith("depth_envelope"):
            last[(r["kind"], r["case"])] = r
    rows = sorted((r for (k, _), r in last.items() if k == "depth_envelope"), key=lambda r: (r["D"], r["th"], r["depth_set"]))
    print("| D | cut-off | depth set | V | K | rays with every sample inside | kept at index 0 / D - 1 | same sets | flips | rel_H | rel_b | oracle jitter rel_H | fp64 check |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %g | %s | %d | %d | %d | %d / %d | %s | %d | %.2e | %.2e | %.2e | %s |" % (
            r["D"], r["th"], r["depth_set"], r["V"], r["K"], r["full_rays"], r["kept_first"], r["kept_last"], "yes" if r["same_sets"] else "NO",
            len(r["named_flips"]) if r["named_flips"] else r["flips"], r["rel_H"], r["rel_b"], r["oracle_jitter_rel_H"], "yes" if r.get("fp64") else "-"))
    passes = sorted((r for (k, _), r in last.items() if k == "depth_envelope_passes"), key=lambda r: r["D"])
    if passes:
        print("\n| D | automatic passes: decoded / in-sphere | one pass: decoded / in-sphere |")
        print("|---|---|---|")
        for r in passes:
            print("| %d | %d / %d = %.3f | %d / %d = %.3f |" % (r["D"], r["fwd"], r["insphere"], r["fwd"] / r["insphere"], r["one_pass_fwd"], r["insphere"],
                                                           r["one_pass_fwd"] / r["insphere"]))


if __name__ == "__main__":
    main()
