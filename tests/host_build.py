"""Compile and run the stand-alone host drivers under tests/host/ with a host sanitizer (CPU machines only; nothing is loaded into Python)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsp_slam_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
CLANGS = ("clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
COMPILERS = ("g++",) + CLANGS


def skip_on_gpu_machine():
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU machine: sanitizer binaries run on CPU machines only")


def compile_driver(sources, sanitize, out, extra=(), compilers=COMPILERS):
    """The first local C++ compiler of `compilers` that accepts -fsanitize=<sanitize> builds `sources` into `out`; skips the test when none does."""
    probe = os.path.join(os.path.dirname(out), "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for cand in compilers:
        cxx = shutil.which(cand)
        if not cxx:
            continue
        flags = ["-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-pthread"]
        if subprocess.run([cxx] + flags + [probe, "-o", probe + ".out"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
            continue
        r = subprocess.run([cxx] + flags + list(extra) + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")] + list(sources) + ["-o", out],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, "%s failed on %s:\n%s" % (cxx, sources, r.stdout)
        return out
    pytest.skip("no local C++ compiler accepts -fsanitize=" + sanitize)


def run_driver(cmd):
    """Runs a driver; it passes when it exits 0 and no sanitizer wrote a report."""
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, "%s: exit %d\n%s\n%s" % (
        cmd[0], r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout
