"""The decoder packers (dsp_slam_amd/csrc/decoder_pack.hip) as a stand-alone program under -fsanitize=address,undefined, tied to the
shipped library by hashes.

tests/host/pack_driver.cpp compiles the packing unit into itself (no libdspgn, no device), fills a decoder from the integer recurrence
below and prints a 64-bit FNV-1a hash of every stream and pass table.  The test feeds the same weights to the loaded library through
dsp_debug_pack, dsp_debug_pack_prepass, dsp_debug_pack_lpj, dsp_debug_split_layout, dsp_debug_cluster_stream and dsp_debug_code_bias
(host-only hooks) and asserts equal hashes, and that no sanitizer reported.
The library's arrays are hashed by the same program (`pack_driver hash`): FNV-1a goes byte by byte, and the streams are tens of megabytes.

Geometries (hidden layers, latent_in, code_len, width): the ones tests/test_pack_emulation.py and tests/test_prepass_emulation.py pack, and
the smallest pack_decoder_host admits.  Its checks want 2 <= latent_in < hidden, so that is THREE hidden layers (latent_in 2, code_len 32,
width 48: the layer in front of latent_in keeps 48 - 35 = 13 outputs); two hidden layers are refused, by the program and the library alike."""
import ctypes as C
import os

import numpy as np
import pytest

import host_build
from dsp_slam_amd import _lib as L

GEOMETRIES = [(8, 4, 64, 512), (8, 4, 32, 512), (8, 4, 64, 256), (8, 4, 32, 256), (8, 4, 64, 384), (6, 3, 64, 512), (7, 4, 64, 512),
              (4, 2, 64, 512), (3, 2, 32, 48), (2, 2, 32, 48), (2, 1, 32, 48)]


def recurrence_layers(hidden, lat, code_len, width, seed):
    """x <- 1664525 x + 1013904223 (mod 2^32) per value, value = (((x >> 9) & 0xFFFF) - 32768) / 2^18; layer by layer, weights before biases.
    (uint32 accumulate wraps mod 2^32: x_n = a^n x_0 + c (1 + a + .. + a^(n-1)).)"""
    in_dim = code_len + 3
    shapes = []
    for k in range(hidden + 1):
        i = in_dim if k == 0 else width
        o = 1 if k == hidden else (width - in_dim if k + 1 == lat else width)
        shapes.append((o, i))
    n = sum(o * i + o for o, i in shapes)
    with np.errstate(over="ignore"):
        a_pow = np.multiply.accumulate(np.full(n, 1664525, np.uint32))                       # a^1 .. a^n
        geo = np.add.accumulate(np.concatenate([np.ones(1, np.uint32), a_pow[:-1]]))          # 1 + a + .. + a^(n-1)
        x = a_pow * np.uint32(seed) + np.uint32(1013904223) * geo
    v = (((x >> np.uint32(9)) & np.uint32(0xFFFF)).astype(np.int32) - 32768).astype(np.float32) / np.float32(262144.0)
    layers, at = [], 0
    for o, i in shapes:
        w = v[at:at + o * i].reshape(o, i)
        b = v[at + o * i:at + o * i + o]
        at += o * i + o
        layers.append((w, b))
    return layers


def test_recurrence_matches_its_statement():
    x, want = 7, []
    for _ in range(200):
        x = (x * 1664525 + 1013904223) % (1 << 32)
        want.append((((x >> 9) & 0xFFFF) - 32768) / 262144.0)
    got = np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in recurrence_layers(3, 2, 3, 16, 7)])
    assert got.dtype == np.float32 and len(got) > 200 and list(got[:200]) == want


def library_arrays(layers, lat, code_len):
    """{name: array, or None where the library refuses the geometry}, in the driver's names and layouts"""
    lib = L.load()
    holder = L.DecoderDescHolder(layers, [lat], code_len)
    out = {}
    slen, blen = C.c_int64(0), C.c_int64(0)
    meta = np.zeros(9, np.int32)
    if lib.dsp_debug_pack(C.byref(holder.desc), None, C.byref(slen), None, C.byref(blen), None, L.ptr(meta, L.c_i32p), None) != 0:
        return {"fp32": None}
    stream, bias, passes, b_last = np.zeros(slen.value, np.float32), np.zeros(blen.value, np.float32), np.zeros((meta[1], 8), np.int32), C.c_float(0)
    L.check(lib.dsp_debug_pack(C.byref(holder.desc), L.ptr(stream), C.byref(slen), L.ptr(bias), C.byref(blen), L.ptr(passes, L.c_i32p),
                               L.ptr(meta, L.c_i32p), C.byref(b_last)), None, "dsp_debug_pack")
    out.update({"fp32.stream": stream, "fp32.bias": bias, "fp32.pass": passes, "fp32.meta": meta, "fp32.b_last": np.array([b_last.value], np.float32)})
    l12, n = np.zeros(12, np.int32), C.c_int64(0)
    L.check(lib.dsp_debug_split_layout(C.byref(holder.desc), L.ptr(l12, L.c_i32p), None, C.byref(n)), None, "dsp_debug_split_layout")
    order = np.zeros(n.value, np.int32)
    L.check(lib.dsp_debug_split_layout(C.byref(holder.desc), L.ptr(l12, L.c_i32p), L.ptr(order, L.c_i32p), C.byref(n)), None, "dsp_debug_split_layout")
    lib.dsp_debug_cluster_stream.restype = C.c_int
    lib.dsp_debug_cluster_stream.argtypes = [C.c_void_p, L.c_i32p, L.c_f32p, L.c_i64p]
    l32, n = np.zeros(32, np.int32), C.c_int64(0)
    L.check(lib.dsp_debug_cluster_stream(C.byref(holder.desc), L.ptr(l32, L.c_i32p), None, C.byref(n)), None, "dsp_debug_cluster_stream")
    cs = np.zeros(n.value, np.float32)
    L.check(lib.dsp_debug_cluster_stream(C.byref(holder.desc), L.ptr(l32, L.c_i32p), L.ptr(cs), C.byref(n)), None, "dsp_debug_cluster_stream")
    code, cb = np.zeros(64, np.float32), np.zeros(1024, np.float32)      # the driver's code: the first code_len weights of layer 0
    code[:code_len] = layers[0][0].reshape(-1)[:code_len]
    L.check(lib.dsp_debug_code_bias(C.byref(holder.desc), L.ptr(code), L.ptr(cb)), None, "dsp_debug_code_bias")
    out.update({"split.layout": l12, "split.order": order, "cluster.layout": l32, "cluster.stream": cs, "code_bias": cb})
    for hook, n_meta, names in ((lib.dsp_debug_pack_prepass, 2, {L.PREPASS_F16: "lp_f16", L.PREPASS_BF16: "lp_bf16"}),
                                (lib.dsp_debug_pack_lpj, 3, {L.COMPUTE_F16: "lpj_f16", L.COMPUTE_BF16: "lpj_bf16"})):
        for dtype, name in names.items():
            n, m = C.c_int64(0), np.zeros(n_meta, np.int32)
            if hook(C.byref(holder.desc), dtype, None, C.byref(n), None, L.ptr(m, L.c_i32p)) != 0:
                out[name] = None
                continue
            s, p = np.zeros(n.value, np.uint16), np.zeros((m[0], 8), np.int32)
            L.check(hook(C.byref(holder.desc), dtype, s.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(n), L.ptr(p, L.c_i32p), L.ptr(m, L.c_i32p)), None, name)
            out.update({name + ".stream": s, name + ".pass": p, name + ".meta": m})
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    host_build.skip_on_gpu_machine()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")      # HIP's headers, as the library's own build needs them (dsp_internal.h: vector types)
    out = str(tmp_path_factory.mktemp("pack_host") / "pack_driver")
    # the packing unit as plain host C++: HIP's headers for types only, no runtime library linked
    return host_build.compile_driver([host_build.HOST + "/pack_driver.cpp", "-x", "c++", host_build.CSRC + "/decoder_pack.hip"], "address,undefined", out,
                                     extra=["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include")],
                                     compilers=host_build.CLANGS)          # (lp_bits uses _Float16: clang, as for the library itself)


@pytest.mark.parametrize("hidden,lat,code_len,width", GEOMETRIES)
def test_packers_match_the_library_under_asan_ubsan(driver, tmp_path, hidden, lat, code_len, width):
    seed = 1000 * hidden + 100 * lat + code_len + width
    lines = host_build.run_driver([driver, "pack", str(hidden), str(lat), str(code_len), str(width), str(seed)]).split("\n")
    got = dict(ln.split() for ln in lines if ln)
    arrays = library_arrays(recurrence_layers(hidden, lat, code_len, width, seed), lat, code_len)
    assert (hidden >= 3) == (arrays.get("fp32", 0) is not None), "what pack_decoder_host's checks admit"
    names = [k for k, a in arrays.items() if a is not None]
    files = []
    for k in names:
        files.append(str(tmp_path / k))
        np.ascontiguousarray(arrays[k]).tofile(files[-1])
    hashes = host_build.run_driver([driver, "hash"] + files).split() if files else []
    want = dict(zip(names, hashes))
    want.update({k: "refused" for k, a in arrays.items() if a is None})
    for k, h in want.items():
        assert got.get(k) == h, "%s: the stand-alone build gives %s, the library %s" % (k, got.get(k), h)
    assert set(got) == set(want)
