#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?  (No GPU needed.)

    python tools/compare_device_code.py TREE_A TREE_B
    python tools/compare_device_code.py --kernels TREE_A TREE_B

For every .hip file under dsp_slam_amd/csrc of either tree: compile it device-only with the flags dsp_slam_amd/build.py uses for that file,
unbundle the gfx950 code object, and compare
  * the sha256 of the .text and of the .rodata section,
  * the sha256 of the code object's metadata note (kernel names, per-kernel register / LDS / scratch figures, argument layouts).
The bundle as a whole is NOT comparable: its module id is hashed from the input path.  Nothing here looks inside a section; it is a plain
hash comparison.  Prints one line per file and section and exits 1 on any difference.

--kernels: per KERNEL instead of per file -- for a change that ADDS kernels to a file and must leave the existing ones alone.  For every
function symbol of the code object: the sha256 of its own bytes of .text (kernels here are self-contained: every call is inlined, branches
are relative) and of its kernel descriptor (registers, LDS, scratch).  Prints the kernels that differ or exist in one tree only, and a
count of the equal ones; exits 1 if a kernel of TREE_A is missing from TREE_B or differs there (kernels only TREE_B has are listed, not errors).
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


def kernel_hashes(tree, src, work):
    """{kernel name: sha256 of its .text bytes + its descriptor} of one .hip file's gfx950 code object"""
    device_hashes(tree, src, work)                      # leaves the code object in work/dev.co
    co = os.path.join(work, "dev.co")
    secs = {}
    for line in _run([_tool("llvm-readelf"), "-S", "-W", co]).decode().splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[1] in (".text", ".rodata"):
            secs[f[1]] = (int(f[3], 16), int(f[4], 16), int(f[5], 16))      # address, file offset, size
    blob = open(co, "rb").read()
    syms = {}
    for line in _run([_tool("llvm-readelf"), "-s", "-W", co]).decode().splitlines():
        f = line.split()            # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[0].endswith(":") and f[3] in ("FUNC", "OBJECT") and f[6] != "UND":
            syms[f[7]] = (int(f[1], 16), int(f[2], 0), f[3])
    out = {}
    for name, (addr, size, kind) in syms.items():
        if kind != "FUNC" or ".text" not in secs:
            continue
        a0, off, _ = secs[".text"]
        hsh = hashlib.sha256(blob[off + addr - a0: off + addr - a0 + size])
        kd = syms.get(name + ".kd")
        if kd and ".rodata" in secs:
            r0, roff, _ = secs[".rodata"]
            desc = bytearray(blob[roff + kd[0] - r0: roff + kd[0] - r0 + kd[1]])
            desc[16:24] = bytes(8)                      # the entry's offset from the descriptor: where the kernel sits, not what it is
            hsh.update(bytes(desc))
        out[name] = hsh.hexdigest()
    return out


def main_kernels(a, b):
    bad = 0
    for src in sorted(f for f in os.listdir(os.path.join(a, "dsp_slam_amd", "csrc")) if f.endswith(".hip")):
        if not os.path.exists(os.path.join(b, "dsp_slam_amd", "csrc", src)):
            print("%-24s only in %s" % (src, a))
            bad += 1
            continue
        with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
            ka, kb = kernel_hashes(a, src, wa), kernel_hashes(b, src, wb)
        same = [k for k in ka if kb.get(k) == ka[k]]
        for k in sorted(ka):
            if k not in kb:
                print("%-24s MISSING in second tree: %s" % (src, k))
                bad += 1
            elif kb[k] != ka[k]:
                print("%-24s DIFFERS: %s" % (src, k))
                bad += 1
        for k in sorted(set(kb) - set(ka)):
            print("%-24s new in second tree: %s" % (src, k))
        print("%-24s %d of %d kernels of the first tree unchanged" % (src, len(same), len(ka)))
    return 1 if bad else 0


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
    if len(sys.argv) == 4 and sys.argv[1] == "--kernels":
        sys.exit(main_kernels(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])))
