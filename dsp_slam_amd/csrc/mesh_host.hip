// Mesh extraction (marching cubes over decoded volumes, single and batched) and surface projection, with their C ABI.  One file because
// dsp_meshes_refine runs surface_run on the meshes the last dsp_extract_meshes left on the handle.
#include "decoder_calls.h"
#include "decoder_pack.h"
#include "surface_math.h"   // constants only: the arithmetic is compiled in surface_kernels.hip (contraction off)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <utility>
#include <vector>

namespace {

// the marching-cubes case tables, built and uploaded the first time a handle extracts a mesh
void ensure_mc_tables(dsp_handle* h) {
    if (h->mc_tab.p) return;
    McTables t;
    mc_build_tables(t);
    h->mc_tab.alloc(1);
    HIP_TRY(hipMemcpy(h->mc_tab.p, &t, sizeof t, hipMemcpyHostToDevice));
}

// marching cubes over a device-resident volume; the mesh stays in h->mc_verts / mc_faces until dsp_mesh_fetch
void extract_mesh_device(dsp_handle* h, const float* vol, int n0, int n1, int n2, float level, float spacing, float origin) {
    if ((int64_t)n0 * n1 * n2 > ((int64_t)1 << 30)) throw std::invalid_argument("volume too large");
    const int n_pts = n0 * n1 * n2;
    ensure_mc_tables(h);
    h->mc_blocks.ensure(mc_num_blocks(n_pts));
    h->mc_totals.ensure(2);
    h->mesh_nv = h->mesh_nf = -1;
    HIP_TRY(launch_mc_count(vol, n0, n1, n2, level, h->mc_tab.p, h->mc_blocks.p, h->mc_totals.p, h->stream));
    long long tot[2];
    HIP_TRY(hipMemcpyAsync(tot, h->mc_totals.p, sizeof tot, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (tot[0] > ((long long)1 << 30) || tot[1] > ((long long)1 << 30)) throw std::invalid_argument("mesh too large");
    h->mc_verts.ensure((size_t)std::max<long long>(tot[0], 1) * 3);
    h->mc_faces.ensure((size_t)std::max<long long>(tot[1], 1) * 3);
    h->mc_vidmap.ensure((size_t)n_pts * 3);
    if (tot[0] > 0)
        HIP_TRY(launch_mc_emit(vol, n0, n1, n2, level, h->mc_tab.p, h->mc_blocks.p, spacing, origin, h->mc_verts.p, h->mc_vidmap.p,
                               h->mc_faces.p, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->mesh_nv = tot[0];
    h->mesh_nf = tot[1];
}

// ------------------------------------------------------------------------------------------------
// batched mesh extraction (dsp_extract_meshes; DESIGN.md "Mesh extraction")
// ------------------------------------------------------------------------------------------------

// grow a device buffer to at least `need` elements, keeping its first `used` ones
template <class T>
void grow_keep(dsp_handle* h, DevBuf<T>& b, size_t used, size_t need) {
    if (need <= b.n) return;
    DevBuf<T> nb;
    nb.alloc(need + need / 4);
    if (used) HIP_TRY(hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::swap(b.p, nb.p);
    std::swap(b.n, nb.n);
    std::swap(b.pool, nb.pool);
    std::swap(b.bytes, nb.bytes);
}

// objects per chunk: chunk volumes + vertex-id maps (+ the band lists with a prepass) within this budget, whatever the device has free
constexpr size_t MESH_CHUNK_BYTES = (size_t)384 << 20;

// n_codes objects on one vol_dim^3 grid -> their meshes, concatenated in `verts` / `faces` (object order; face indices local to their
// mesh), counts in nv / nf.  lp: 0 = every grid point through the fp32 kernel; 1 / 2 = f16 / bf16 prepass over every point, the fp32
// kernel over the surface band (k_mesh_band) only, the guard on what it re-decodes; an object whose guard trips is decoded densely in
// fp32 again before marching cubes.  delta > 0: that margin for every object, else the calibrated one of its code (lp_delta_host; the
// handle's table is read, never changed).  Statistics of the call in h->ms_*.
void extract_meshes_impl(dsp_handle* h, const float* codes, int64_t n_codes, int vol_dim, bool regular, int lp, float delta,
                         DevBuf<float>& verts, DevBuf<int>& faces, std::vector<int64_t>& nv, std::vector<int64_t>& nf) {
    if (lp && !h->lp_ok)
        throw std::invalid_argument("this decoder's geometry has no prepass kernel (it needs an even number of hidden layers, one latent_in "
                                    "layer, width <= 512): mesh extraction with a prepass flag is not available");
    const int n = vol_dim;
    const int64_t n_pts = (int64_t)n * n * n;
    const float voxel_size = (float)(2.0 / (vol_dim - 1));
    for (auto& c : h->ms_counts) c = 0;
    h->ms_max_err = 0.f;
    nv.assign((size_t)n_codes, 0);
    nf.assign((size_t)n_codes, 0);
    HIP_TRY(hipSetDevice(h->device));
    const size_t per_obj = (size_t)n_pts * (4 + 12 + (lp ? sizeof(float4) + 4 + 8 : 0));     // volume, vidmap (+ band point, value, index)
    int64_t chunk = std::max<int64_t>(1, (int64_t)(MESH_CHUNK_BYTES / per_obj));
    chunk = std::min<int64_t>(chunk, (((int64_t)1 << 31) - 1) / n_pts);    // int point indices inside a chunk (tile lists, decode request)
    chunk = std::min<int64_t>(std::min<int64_t>(chunk, 1024), n_codes);   // k_mesh_tile_scan: one block
    ensure_mc_tables(h);
    h->s_pts.ensure(n_pts);
    HIP_TRY(launch_grid_points(h->s_pts.p, n, voxel_size, regular ? 1 : 0, h->stream));     // one grid for every object
    LpDeltaTab tab{};
    if (lp) {
        const int bf = lp == DSP_PREPASS_BF16 ? 1 : 0;
        tab = h->lp_tab[bf];
        for (int m = 0; m < LP_NMAG; ++m) tab.delta[m] = std::min(0.5f, std::max(tab.delta[m], 4.f * h->lp_guard_err[bf]));
    }
    const int nb = mc_num_blocks((int)n_pts);
    const int64_t tiles_per_obj = (n_pts + MESH_TILE_PTS - 1) / MESH_TILE_PTS;
    size_t out_v = 0, out_f = 0;
    for (int64_t c0 = 0; c0 < n_codes; c0 += chunk) {
        const int nc = (int)std::min<int64_t>(chunk, n_codes - c0);
        const float* cc = codes + c0 * CODE_LEN;
        h->mb_vol.ensure((size_t)nc * n_pts);
        float* vol = h->mb_vol.p;
        if (!lp) {
            decode_resident_points(h, cc, nc, n_pts, false, 0, vol);
            h->ms_counts[3] += (int64_t)nc * n_pts;
        } else {
            std::vector<unsigned> gw((size_t)3 * nc, 0u);
            std::vector<int> cnt((size_t)2 * nc);
            for (int c = 0; c < nc; ++c) {
                const float d = delta > 0.f ? delta : lp_delta_host(cc + (size_t)c * CODE_LEN, tab);
                memcpy(&gw[3 * c], &d, 4);
            }
            h->mb_guard.ensure((size_t)3 * nc);
            h->mb_cnt.ensure((size_t)3 * nc + 1);
            h->mb_pts.ensure((size_t)nc * n_pts);
            h->mb_val.ensure((size_t)nc * n_pts);
            h->mb_idx.ensure((size_t)nc * n_pts);
            h->mb_tiles.ensure((size_t)nc * tiles_per_obj);
            HIP_TRY(hipMemcpyAsync(h->mb_guard.p, gw.data(), gw.size() * 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemsetAsync(h->mb_cnt.p, 0, (size_t)2 * nc * 4, h->stream));
            // prepass over every grid point of every object (one launch); uploads the chunk's codes and code biases (s_code, s_cbias) --
            // the ones the fp32 launch below uses, as the dense path does -- and synchronises after them (gw is still alive)
            decode_resident_points(h, cc, nc, n_pts, false, lp, vol);
            int* d_cnt = h->mb_cnt.p;
            HIP_TRY(launch_mesh_band(vol, h->s_pts.p, n, nc, h->mb_guard.p, h->mb_pts.p, h->mb_val.p, h->mb_idx.p, d_cnt, d_cnt + 2 * nc,
                                     d_cnt + 3 * nc, h->mb_tiles.p, h->stream));
            MlpArgs a = make_mlp_args(h, 0);
            a.n_tiles = d_cnt + 3 * nc;
            a.tiles = h->mb_tiles.p;
            a.pts = h->mb_pts.p;
            a.code_bias = h->s_cbias.p;
            a.code_bias_stride = 2 * WIDTH;
            a.out_sdf = h->mb_val.p;        // pre-filled with the prepass values: the guard compares them with the fp32 values it stores
            a.guard = h->mb_guard.p;
            a.guard_stride = 3;
            a.clk = h->s_clk.p;
            HIP_TRY(launch_mlp(0, a, (int)std::min<int64_t>((int64_t)nc * tiles_per_obj, h->n_cu), h->stream));
            HIP_TRY(launch_mesh_scatter(h->mb_val.p, h->mb_idx.p, d_cnt, n, nc, vol, h->stream));
            HIP_TRY(hipMemcpyAsync(gw.data(), h->mb_guard.p, gw.size() * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            h->ms_counts[0] += (int64_t)nc * n_pts;
            for (int c = 0; c < nc; ++c) {
                h->ms_counts[1] += cnt[c] - cnt[nc + c];
                h->ms_counts[2] += cnt[nc + c];
                float e;
                memcpy(&e, &gw[3 * c + 2], 4);
                if (!(e <= h->ms_max_err)) h->ms_max_err = e;
                if (gw[3 * c + 1] != 0u) {      // tripped: this object's volume densely in fp32 (the margin table stays as it is)
                    decode_resident_points(h, cc + (size_t)c * CODE_LEN, 1, n_pts, false, 0, vol + (size_t)c * n_pts);
                    h->ms_counts[3] += n_pts;
                    h->ms_counts[4] += 1;
                }
            }
        }
        // marching cubes over the chunk's volumes
        h->mc_blocks.ensure((size_t)nb * nc);
        h->mc_totals.ensure(2);
        h->mb_base.ensure(nc);
        HIP_TRY(launch_mc_count_batched(vol, n, nc, 0.f, h->mc_tab.p, h->mc_blocks.p, h->mc_totals.p, h->mb_base.p, h->stream));
        long long tot[2];
        std::vector<int2> base(nc);
        HIP_TRY(hipMemcpyAsync(tot, h->mc_totals.p, sizeof tot, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(base.data(), h->mb_base.p, nc * sizeof(int2), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (tot[0] > ((long long)1 << 30) || tot[1] > ((long long)1 << 30)) throw std::invalid_argument("meshes too large (split the request)");
        for (int c = 0; c < nc; ++c) {
            nv[c0 + c] = (c + 1 < nc ? base[c + 1].x : tot[0]) - base[c].x;
            nf[c0 + c] = (c + 1 < nc ? base[c + 1].y : tot[1]) - base[c].y;
        }
        grow_keep(h, verts, 3 * out_v, 3 * (out_v + std::max<long long>(tot[0], 1)));
        grow_keep(h, faces, 3 * out_f, 3 * (out_f + std::max<long long>(tot[1], 1)));
        h->mc_vidmap.ensure((size_t)nc * 3 * n_pts);
        if (tot[0] > 0)
            HIP_TRY(launch_mc_emit_batched(vol, n, nc, 0.f, h->mc_tab.p, h->mc_blocks.p, voxel_size, -1.f, verts.p + 3 * out_v, h->mc_vidmap.p,
                                           faces.p + 3 * out_f, h->stream));
        out_v += tot[0];
        out_f += tot[1];
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
}

// ------------------------------------------------------------------------------------------------
// surface projection (dsp_surface_points, dsp_meshes_refine; arithmetic: surface_math.h, kernels: surface_kernels.hip)
// ------------------------------------------------------------------------------------------------

// rows of the decoder's output (GRAD_STRIDE floats each) one chunk may hold, whatever the device has free
constexpr size_t SURFACE_CHUNK_BYTES = (size_t)64 << 20;

// validated copy of a caller's variances as the kernels read them: n_codes x 64 floats, entries at or beyond the decoder's code length zero
std::vector<float> surface_variances(const dsp_handle* h, const double* var_code, int64_t n_codes) {
    std::vector<float> v((size_t)n_codes * CODE_LEN, 0.f);
    for (int64_t c = 0; c < n_codes; ++c)
        for (int k = 0; k < h->code_len; ++k) {
            const double x = var_code[c * CODE_LEN + k];
            if (!(x >= 0.0) || !std::isfinite(x)) throw std::invalid_argument("var_code entries must be finite and >= 0");
            v[(size_t)c * CODE_LEN + k] = (float)x;
        }
    return v;
}

struct SurfaceOut {             // device arrays over ALL points of the call, in the order of the inputs; any may be null
    float *pts = nullptr, *normals = nullptr, *sdf = nullptr, *grad_norm = nullptr, *sigma = nullptr;
};

// Object c owns the points [off[c], off[c + 1]) of pts3 (device, packed float3, object frame).  n_steps x (mlp_kernel<2>, k_surface_step),
// then mlp_kernel<2> + k_surface_attributes, in chunks of at most the budget's rows; a chunk may end inside an object (its tiles then start
// at the chunk's first point of that object).  var: host, n_codes x 64 floats (surface_variances) or null.  Scratch is the single-shot
// decoder calls' (s_pts, s_out, s_tiles, s_cbias) plus sf_var, all from the handle's pool.  Synchronises before it returns.
void surface_run(dsp_handle* h, const float* codes, int64_t n_codes, const int64_t* off, const float* pts3, int n_steps, float max_step,
                 const float* var, const SurfaceOut& out) {
    const int64_t total = off[n_codes];
    if (total <= 0) return;
    HIP_TRY(hipSetDevice(h->device));
    const int64_t budget = h->sf_chunk_rows > 0 ? h->sf_chunk_rows : (int64_t)(SURFACE_CHUNK_BYTES / (GRAD_STRIDE * sizeof(float)));
    const int64_t rows = std::min<int64_t>(budget, total);
    h->s_pts.ensure((size_t)rows);
    h->s_out.ensure((size_t)rows * GRAD_STRIDE);
    h->s_ntiles.ensure(1);
    h->s_clk.ensure(4);
    std::vector<int4> tiles;
    std::vector<float> cb, vv;
    int64_t c = 0;
    for (int64_t s = 0; s < total; s += rows) {
        const int64_t e = std::min(total, s + rows);
        const int n = (int)(e - s);
        while (off[c + 1] <= s) ++c;            // first object with a point in [s, e)
        const int64_t c0 = c;
        tiles.clear();
        int64_t c1 = c0;
        for (int64_t o = c0; o < n_codes && off[o] < e; ++o) {
            const int64_t a = std::max(off[o], s), b = std::min(off[o + 1], e);
            for (int64_t i = a; i < b; i += TILE_PTS)
                tiles.push_back(make_int4((int)(i - s), (int)std::min<int64_t>(TILE_PTS, b - i), (int)(o - c0), 0));
            if (b > a) c1 = o + 1;
        }
        const int64_t nc = c1 - c0;
        const int nt = (int)tiles.size();
        cb.resize((size_t)2 * WIDTH * nc);
        for (int64_t o = 0; o < nc; ++o) code_bias_host(h->h_codew, h->h_b0, h->h_blat, codes + (c0 + o) * CODE_LEN, cb.data() + o * 2 * WIDTH);
        h->s_cbias.ensure(cb.size());
        h->s_tiles.ensure(nt);
        if (var) h->sf_var.ensure((size_t)nc * CODE_LEN);
        HIP_TRY(hipMemcpyAsync(h->s_cbias.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->s_tiles.p, tiles.data(), nt * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->s_ntiles.p, &nt, 4, hipMemcpyHostToDevice, h->stream));
        if (var) HIP_TRY(hipMemcpyAsync(h->sf_var.p, var + (size_t)c0 * CODE_LEN, (size_t)nc * CODE_LEN * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));     // the staging vectors are refilled by the next chunk
        HIP_TRY(launch_surface_pack(pts3 + 3 * s, h->s_pts.p, nullptr, n, 0, h->stream));
        MlpArgs a = make_mlp_args(h, 2);
        a.n_tiles = h->s_ntiles.p;
        a.tiles = h->s_tiles.p;
        a.pts = h->s_pts.p;
        a.code_bias = h->s_cbias.p;
        a.code_bias_stride = 2 * WIDTH;
        a.out_sdf = h->s_out.p;
        a.out_grad = h->s_out.p;
        a.clk = h->s_clk.p;
        const int n_blocks = std::min(nt, h->n_cu);
        for (int k = 0; k < n_steps; ++k) {
            HIP_TRY(launch_mlp(2, a, n_blocks, h->stream));
            HIP_TRY(launch_surface_step(h->s_pts.p, h->s_out.p, n, max_step, h->stream));
        }
        HIP_TRY(launch_mlp(2, a, n_blocks, h->stream));
        HIP_TRY(launch_surface_attributes(h->s_tiles.p, nt, h->s_pts.p, h->s_out.p, var ? h->sf_var.p : nullptr, out.normals ? out.normals + 3 * s : nullptr,
                                          out.grad_norm ? out.grad_norm + s : nullptr, out.sdf ? out.sdf + s : nullptr,
                                          out.sigma ? out.sigma + s : nullptr, h->stream));
        if (out.pts) HIP_TRY(launch_surface_pack(nullptr, h->s_pts.p, out.pts + 3 * s, n, 1, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
}

}  // namespace

extern "C" {

namespace {
// DSP_MESH_PREPASS_* bits of a flags word -> 0 (none) / DSP_PREPASS_F16 / DSP_PREPASS_BF16; -1 = unknown bits or both dtypes
int mesh_flags_lp(int32_t flags) {
    if (flags & ~(DSP_MESH_REGULAR_GRID | DSP_MESH_PREPASS_F16 | DSP_MESH_PREPASS_BF16)) return -1;
    const bool f16 = (flags & DSP_MESH_PREPASS_F16) != 0, bf16 = (flags & DSP_MESH_PREPASS_BF16) != 0;
    if (f16 && bf16) return -1;
    return f16 ? DSP_PREPASS_F16 : bf16 ? DSP_PREPASS_BF16 : 0;
}
}  // namespace

int dsp_extract_mesh(dsp_handle* h, const float* code, int32_t vol_dim, int32_t flags, int64_t* n_vertices, int64_t* n_faces) {
    const int lp = mesh_flags_lp(flags);
    if (!h || !code || vol_dim < 2 || vol_dim > 512 || !n_vertices || !n_faces || lp < 0) return DSP_E_ARG;
    if (lp) {
        return guarded(h, [&] {
            h->mesh_nv = h->mesh_nf = -1;
            std::vector<int64_t> nv, nf;
            extract_meshes_impl(h, code, 1, vol_dim, (flags & DSP_MESH_REGULAR_GRID) != 0, lp, 0.f, h->mc_verts, h->mc_faces, nv, nf);
            h->mesh_nv = *n_vertices = nv[0];
            h->mesh_nf = *n_faces = nf[0];
        });
    }
    return guarded(h, [&] {
        HIP_TRY(hipSetDevice(h->device));
        const int64_t n = (int64_t)vol_dim * vol_dim * vol_dim;
        const float voxel_size = (float)(2.0 / (vol_dim - 1));
        h->s_pts.ensure(n);
        HIP_TRY(launch_grid_points(h->s_pts.p, vol_dim, voxel_size, (flags & DSP_MESH_REGULAR_GRID) ? 1 : 0, h->stream));
        decode_resident_points(h, code, 1, n, false);
        for (auto& c : h->ms_counts) c = 0;
        h->ms_counts[3] = n;
        h->ms_max_err = 0.f;
        extract_mesh_device(h, h->s_out.p, vol_dim, vol_dim, vol_dim, 0.f, voxel_size, -1.f);
        *n_vertices = h->mesh_nv;
        *n_faces = h->mesh_nf;
    });
}

int dsp_marching_cubes(dsp_handle* h, const float* volume, int32_t n0, int32_t n1, int32_t n2, float level, float spacing, float origin,
                       int64_t* n_vertices, int64_t* n_faces) {
    if (!h || !volume || n0 < 2 || n1 < 2 || n2 < 2 || !n_vertices || !n_faces) return DSP_E_ARG;
    return guarded(h, [&] {
        HIP_TRY(hipSetDevice(h->device));
        const size_t n = (size_t)n0 * n1 * n2;
        h->mc_vol.ensure(n);
        HIP_TRY(hipMemcpyAsync(h->mc_vol.p, volume, n * 4, hipMemcpyHostToDevice, h->stream));
        extract_mesh_device(h, h->mc_vol.p, n0, n1, n2, level, spacing, origin);
        *n_vertices = h->mesh_nv;
        *n_faces = h->mesh_nf;
    });
}

int dsp_mesh_fetch(dsp_handle* h, float* vertices, int64_t n_vertices, int32_t* faces, int64_t n_faces) {
    if (!h || n_vertices < 0 || n_faces < 0 || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return DSP_E_ARG;
    return guarded(h, [&] {
        // the counts are read under the handle's lock and must be the ones the caller sized its buffers for: another thread's
        // dsp_extract_mesh between this caller's extract and fetch is reported, never copied into the wrong-sized buffers
        if (h->mesh_nv < 0 || h->mesh_nv != n_vertices || h->mesh_nf != n_faces)
            throw state_error("no mesh of that size on this handle (another extract ran in between?)");
        HIP_TRY(hipSetDevice(h->device));
        if (h->mesh_nv > 0) HIP_TRY(hipMemcpyAsync(vertices, h->mc_verts.p, (size_t)h->mesh_nv * 12, hipMemcpyDeviceToHost, h->stream));
        if (h->mesh_nf > 0) HIP_TRY(hipMemcpyAsync(faces, h->mc_faces.p, (size_t)h->mesh_nf * 12, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    });
}

int dsp_extract_meshes(dsp_handle* h, const float* codes, int64_t n_codes, int32_t vol_dim, int32_t flags, float delta, int64_t* n_vertices,
                       int64_t* n_faces) {
    const int lp = mesh_flags_lp(flags);
    if (!h || !codes || n_codes < 1 || vol_dim < 2 || vol_dim > 512 || !n_vertices || !n_faces || lp < 0 || !(delta == delta)) return DSP_E_ARG;
    return guarded(h, [&] {
        h->mm_valid = false;
        h->mr_valid = false;
        extract_meshes_impl(h, codes, n_codes, vol_dim, (flags & DSP_MESH_REGULAR_GRID) != 0, lp, delta, h->mm_verts, h->mm_faces, h->mm_nv, h->mm_nf);
        h->mm_codes.assign(codes, codes + n_codes * CODE_LEN);
        h->mm_voxel = (float)(2.0 / (vol_dim - 1));
        h->mm_valid = true;
        memcpy(n_vertices, h->mm_nv.data(), n_codes * 8);
        memcpy(n_faces, h->mm_nf.data(), n_codes * 8);
    });
}

int dsp_meshes_fetch(dsp_handle* h, int64_t n_codes, const int64_t* n_vertices, const int64_t* n_faces, float* vertices, int32_t* faces) {
    if (!h || n_codes < 1 || !n_vertices || !n_faces) return DSP_E_ARG;
    return guarded(h, [&] {
        if (!h->mm_valid || (int64_t)h->mm_nv.size() != n_codes) throw state_error("no batched meshes of that size on this handle (another extract ran in between?)");
        int64_t tv = 0, tf = 0;
        for (int64_t c = 0; c < n_codes; ++c) {
            if (h->mm_nv[c] != n_vertices[c] || h->mm_nf[c] != n_faces[c])
                throw state_error("no batched meshes of that size on this handle (another extract ran in between?)");
            tv += n_vertices[c];
            tf += n_faces[c];
        }
        if ((tv > 0 && !vertices) || (tf > 0 && !faces)) throw std::invalid_argument("null output buffer");
        HIP_TRY(hipSetDevice(h->device));
        if (tv > 0) HIP_TRY(hipMemcpyAsync(vertices, h->mm_verts.p, (size_t)tv * 12, hipMemcpyDeviceToHost, h->stream));
        if (tf > 0) HIP_TRY(hipMemcpyAsync(faces, h->mm_faces.p, (size_t)tf * 12, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    });
}

int dsp_mesh_last_stats(dsp_handle* h, int64_t* counts5, float* max_guard_err) {
    if (!h || !counts5) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    memcpy(counts5, h->ms_counts, sizeof h->ms_counts);
    if (max_guard_err) *max_guard_err = h->ms_max_err;
    return DSP_OK;
}

namespace {
bool surface_steps_ok(int32_t n_steps) { return n_steps >= 0 && n_steps <= surface_math::MAX_STEPS; }
}  // namespace

int dsp_surface_points(dsp_handle* h, const float* codes, int64_t n_codes, const int64_t* pts_off, const float* pts, int32_t n_steps, float max_step,
                       const double* var_code, float* pts_out, float* normals, float* sdf, float* grad_norm, float* sigma) {
    if (!h || !codes || n_codes < 1 || !pts_off || !surface_steps_ok(n_steps) || !std::isfinite(max_step) || !(max_step > 0.f)) return DSP_E_ARG;
    if (pts_off[0] != 0) return DSP_E_ARG;
    for (int64_t c = 0; c < n_codes; ++c)
        if (pts_off[c + 1] < pts_off[c]) return DSP_E_ARG;
    const int64_t total = pts_off[n_codes];
    if ((total > 0 && !pts) || (sigma && !var_code)) return DSP_E_ARG;
    return guarded(h, [&] {
        std::vector<float> var;
        if (var_code) var = surface_variances(h, var_code, n_codes);
        if (total == 0) return;
        HIP_TRY(hipSetDevice(h->device));
        DevBuf<float> d_in, d_pts, d_nrm, d_sdf, d_gn, d_sig;
        d_in.alloc((size_t)total * 3);
        SurfaceOut out;
        if (pts_out) { d_pts.alloc((size_t)total * 3); out.pts = d_pts.p; }
        if (normals) { d_nrm.alloc((size_t)total * 3); out.normals = d_nrm.p; }
        if (sdf) { d_sdf.alloc((size_t)total); out.sdf = d_sdf.p; }
        if (grad_norm) { d_gn.alloc((size_t)total); out.grad_norm = d_gn.p; }
        if (sigma) { d_sig.alloc((size_t)total); out.sigma = d_sig.p; }
        HIP_TRY(hipMemcpyAsync(d_in.p, pts, (size_t)total * 12, hipMemcpyHostToDevice, h->stream));
        surface_run(h, codes, n_codes, pts_off, d_in.p, n_steps, max_step, var_code ? var.data() : nullptr, out);
        if (pts_out) HIP_TRY(hipMemcpyAsync(pts_out, d_pts.p, (size_t)total * 12, hipMemcpyDeviceToHost, h->stream));
        if (normals) HIP_TRY(hipMemcpyAsync(normals, d_nrm.p, (size_t)total * 12, hipMemcpyDeviceToHost, h->stream));
        if (sdf) HIP_TRY(hipMemcpyAsync(sdf, d_sdf.p, (size_t)total * 4, hipMemcpyDeviceToHost, h->stream));
        if (grad_norm) HIP_TRY(hipMemcpyAsync(grad_norm, d_gn.p, (size_t)total * 4, hipMemcpyDeviceToHost, h->stream));
        if (sigma) HIP_TRY(hipMemcpyAsync(sigma, d_sig.p, (size_t)total * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));     // before the device blocks go back to the pool
    });
}

int dsp_meshes_refine(dsp_handle* h, int64_t n_codes, const int64_t* n_vertices, int32_t n_steps, float max_step, const double* var_code) {
    if (!h || n_codes < 1 || !n_vertices || !surface_steps_ok(n_steps) || !std::isfinite(max_step)) return DSP_E_ARG;
    return guarded(h, [&] {
        if (!h->mm_valid || (int64_t)h->mm_nv.size() != n_codes) throw state_error("no batched meshes of that size on this handle (another extract ran in between?)");
        std::vector<int64_t> off((size_t)n_codes + 1, 0);
        for (int64_t c = 0; c < n_codes; ++c) {
            if (h->mm_nv[c] != n_vertices[c]) throw state_error("no batched meshes of that size on this handle (another extract ran in between?)");
            off[c + 1] = off[c] + n_vertices[c];
        }
        std::vector<float> var;
        if (var_code) var = surface_variances(h, var_code, n_codes);
        h->mr_valid = false;
        const size_t total = (size_t)off[n_codes];
        h->mr_verts.ensure(total * 3);
        h->mr_normals.ensure(total * 3);
        h->mr_sdf.ensure(total);
        if (var_code) h->mr_sigma.ensure(total);
        SurfaceOut out;
        out.pts = h->mr_verts.p;
        out.normals = h->mr_normals.p;
        out.sdf = h->mr_sdf.p;
        out.sigma = var_code ? h->mr_sigma.p : nullptr;
        surface_run(h, h->mm_codes.data(), n_codes, off.data(), h->mm_verts.p, n_steps, max_step > 0.f ? max_step : h->mm_voxel,
                    var_code ? var.data() : nullptr, out);
        h->mr_has_var = var_code != nullptr;
        h->mr_valid = true;
    });
}

int dsp_meshes_fetch_attributes(dsp_handle* h, int64_t n_codes, const int64_t* n_vertices, float* vertices, float* normals, float* sdf, float* sigma) {
    if (!h || n_codes < 1 || !n_vertices) return DSP_E_ARG;
    return guarded(h, [&] {
        if (!h->mm_valid || !h->mr_valid || (int64_t)h->mm_nv.size() != n_codes) throw state_error("no refined meshes of that size on this handle (no dsp_meshes_refine since the last extract?)");
        size_t total = 0;
        for (int64_t c = 0; c < n_codes; ++c) {
            if (h->mm_nv[c] != n_vertices[c]) throw state_error("no refined meshes of that size on this handle (another extract ran in between?)");
            total += (size_t)n_vertices[c];
        }
        if (sigma && !h->mr_has_var) throw state_error("sigma was not computed: dsp_meshes_refine had no var_code");
        if (total == 0) return;
        HIP_TRY(hipSetDevice(h->device));
        if (vertices) HIP_TRY(hipMemcpyAsync(vertices, h->mr_verts.p, total * 12, hipMemcpyDeviceToHost, h->stream));
        if (normals) HIP_TRY(hipMemcpyAsync(normals, h->mr_normals.p, total * 12, hipMemcpyDeviceToHost, h->stream));
        if (sdf) HIP_TRY(hipMemcpyAsync(sdf, h->mr_sdf.p, total * 4, hipMemcpyDeviceToHost, h->stream));
        if (sigma) HIP_TRY(hipMemcpyAsync(sigma, h->mr_sigma.p, total * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    });
}

int dsp_debug_surface_step(int64_t n, const float* pts, const float* sdf, const float* grad_xyz, float max_step, float* pts_out) {
    if (n < 0 || (n > 0 && (!pts || !sdf || !grad_xyz || !pts_out)) || !std::isfinite(max_step) || !(max_step > 0.f)) return DSP_E_ARG;
    surface_step_host(n, pts, sdf, grad_xyz, max_step, pts_out);
    return DSP_OK;
}

int dsp_debug_surface_attributes(int64_t n, const float* rows68, const double* var_code, float* normals, float* grad_norm, float* sdf, float* sigma) {
    if (n < 0 || (n > 0 && !rows68) || (sigma && !var_code)) return DSP_E_ARG;
    float var[CODE_LEN];
    if (var_code)
        for (int k = 0; k < CODE_LEN; ++k) {
            if (!(var_code[k] >= 0.0) || !std::isfinite(var_code[k])) return DSP_E_ARG;
            var[k] = (float)var_code[k];
        }
    surface_attributes_host(n, rows68, var_code ? var : nullptr, normals, grad_norm, sdf, sigma);
    return DSP_OK;
}

int dsp_debug_surface_chunk_rows(dsp_handle* h, int64_t rows) {
    if (!h || rows < 0 || rows > ((int64_t)1 << 24)) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->sf_chunk_rows = rows;
    return DSP_OK;
}

int dsp_debug_mc_table(uint8_t* n_tri, uint8_t* tri) {
    if (!n_tri || !tri) return DSP_E_ARG;
    return guarded(nullptr, [&] {
        McTables t;
        mc_build_tables(t);
        memcpy(n_tri, t.n_tri, 256);
        for (int c = 0; c < 256; ++c) memcpy(tri + c * 3 * MC_MAX_TRI, t.tri[c], 3 * MC_MAX_TRI);
    });
}

}  // extern "C"
