#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?  (No GPU needed.)

    python tools/compare_device_code.py TREE_A TREE_B

For every .hip file under dsp_slam_amd/csrc of either tree: compile it device-only with the flags dsp_slam_amd/build.py uses for that file,
unbundle the gfx950 code object, and compare
  * the sha256 of the .text and of the .rodata section,
  * the sha256 of the code object's metadata note (kernel names, per-kernel register / LDS / scratch figures, argument layouts).
The bundle as a whole is NOT comparable: its module id is hashed from the input path.  Nothing here looks inside a section; it is a plain
hash comparison.  Prints one line per file and section and exits 1 on any difference.
"""
import hashlib
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name):
    for cand in (shutil.which(name), "/opt/rocm/llvm/bin/" + name, "/opt/rocm/lib/llvm/bin/" + name):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError(name + " not found")


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), r.stdout.decode(errors="replace")))
    return r.stdout


def _extra_flags(tree):
    spec = importlib.util.spec_from_file_location("_build_of_tree", os.path.join(tree, "dsp_slam_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.EXTRA_FLAGS


def device_hashes(tree, src, work):
    """{section or 'metadata': sha256} of one .hip file's gfx950 code object"""
    csrc = os.path.join(tree, "dsp_slam_amd", "csrc")
    lib_dir = os.path.join(tree, "dsp_slam_amd", "lib")
    info = os.path.join(work, "info")                   # build_info.h is written by build(); host-only text, but the file must exist
    os.makedirs(info, exist_ok=True)
    if not os.path.exists(os.path.join(lib_dir, "build_info.h")):
        with open(os.path.join(info, "build_info.h"), "w") as f:
            f.write('#define DSP_BUILD_HIPCC "compare"\n')
    bundle, co = os.path.join(work, "dev.bundle"), os.path.join(work, "dev.co")
    _run([_tool("hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-Wno-unused-value", "--offload-device-only",
          "-I" + os.path.join(tree, "include"), "-I" + csrc, "-I" + lib_dir, "-I" + info] + _extra_flags(tree).get(src, []) +
         [os.path.join(csrc, src), "-o", bundle])
    _run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + co])
    out = {}
    for sec in (".text", ".rodata"):
        dump = os.path.join(work, "sec.bin")
        if os.path.exists(dump):
            os.remove(dump)
        try:
            _run([_tool("llvm-objcopy"), "--dump-section", "%s=%s" % (sec, dump), co, os.path.join(work, "unused.co")])
        except RuntimeError as e:
            if "not found" not in str(e):
                raise
            out[sec] = "absent"         # a file without kernels, or without constants
            continue
        with open(dump, "rb") as f:
            out[sec] = hashlib.sha256(f.read()).hexdigest()
    out["metadata"] = hashlib.sha256(_run([_tool("llvm-readelf"), "--notes", co])).hexdigest()
    return out


def main(a, b):
    def hips(t):
        return {f for f in os.listdir(os.path.join(t, "dsp_slam_amd", "csrc")) if f.endswith(".hip")}
    differ = 0
    for src in sorted(hips(a) | hips(b)):
        if src not in hips(a) or src not in hips(b):
            print("%-24s only in one tree" % src)
            differ += 1
            continue
        with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
            ha, hb = device_hashes(a, src, wa), device_hashes(b, src, wb)
        for key in sorted(ha):
            same = ha[key] == hb[key]
            differ += not same
            print("%-24s %-9s %s %s" % (src, key, ha[key][:16], "same" if same else "DIFFERS from " + hb[key][:16]))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])))
