// Stand-alone driver for the decoder packers (dsp_slam_amd/csrc/decoder_pack.hip, compiled into this program as plain host C++ with
// -fsanitize=address,undefined by tests/test_pack_host.py).  No libdspgn, no device.
//   pack_driver pack HIDDEN LATENT_IN CODE_LEN WIDTH SEED   one decoder filled from the recurrence below through every packer: one line
//                                                            "<name> <FNV-1a 64 of the bytes>" per stream and table, in the layout of the
//                                                            dsp_debug_pack* hooks; "<name> refused" where a packer does not take the geometry
//   pack_driver hash FILE...                                 "<FNV-1a 64>" of every file's bytes (the test hashes the library's arrays with it)
#include "decoder_pack.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

using namespace dsp;
using namespace dsp_host;

static uint64_t fnv1a(const void* data, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}
static void line(const std::string& name, const void* data, size_t n) { printf("%s %016llx\n", name.c_str(), (unsigned long long)fnv1a(data, n)); }

// the weights: x <- 1664525 x + 1013904223 (mod 2^32) per value, value = (((x >> 9) & 0xFFFF) - 32768) / 2^18; layer by layer, a layer's
// weights (row-major [out][in]) before its biases.  tests/test_pack_host.py states the same recurrence.
struct Net {
    std::vector<std::vector<float>> w, b;
    std::vector<int32_t> out_dims, in_dims;
    std::vector<const float*> wp, bp;
    dsp_decoder_desc desc;
    Net(int hidden, int lat, int code_len, int width, uint32_t seed) {
        uint32_t x = seed;
        auto next = [&]() { x = x * 1664525u + 1013904223u; return (float)((int)((x >> 9) & 0xFFFF) - 32768) / 262144.f; };
        const int in_dim = code_len + 3;
        for (int k = 0; k <= hidden; ++k) {
            const int id = k == 0 ? in_dim : width, od = k == hidden ? 1 : (k + 1 == lat ? width - in_dim : width);
            in_dims.push_back(id);
            out_dims.push_back(od);
            w.emplace_back((size_t)od * id);
            b.emplace_back((size_t)od);
            for (float& v : w.back()) v = next();
            for (float& v : b.back()) v = next();
        }
        for (int k = 0; k <= hidden; ++k) { wp.push_back(w[k].data()); bp.push_back(b[k].data()); }
        memset(&desc, 0, sizeof desc);
        desc.n_layers = hidden + 1;
        desc.code_len = code_len;
        desc.latent_in = lat;
        desc.out_dims = out_dims.data();
        desc.in_dims = in_dims.data();
        desc.weights = wp.data();
        desc.biases = bp.data();
    }
};

static void lp_lines(const std::string& name, bool ok, const PackedLp& pl, const std::vector<int32_t>& meta) {
    if (!ok) { printf("%s refused\n", name.c_str()); return; }
    std::vector<int32_t> pass((size_t)pl.n_pass * 8);
    for (int i = 0; i < pl.n_pass; ++i) {
        const LpPass& q = pl.pass[i];
        const int32_t o[8] = {q.nog, q.nchunks, q.bias_row, q.kind, q.npad, q.last, q.chunk_base, 0};
        memcpy(&pass[(size_t)i * 8], o, sizeof o);
    }
    line(name + ".stream", pl.stream.data(), pl.stream.size() * 2);
    line(name + ".pass", pass.data(), pass.size() * 4);
    line(name + ".meta", meta.data(), meta.size() * 4);
}

static int pack(int hidden, int lat, int code_len, int width, uint32_t seed) {
    Net net(hidden, lat, code_len, width, seed);
    PackedNet pn;
    try {
        pack_decoder_host(&pn, &net.desc);
    } catch (const std::invalid_argument&) {
        printf("fp32 refused\n");
        return 0;
    }
    std::vector<int32_t> pass((size_t)pn.n_pass_all * 8);
    for (int i = 0; i < pn.n_pass_all; ++i) {
        const PassDesc& p = pn.pass[i];
        const int32_t o[8] = {p.nog, p.nchunks, p.bias_row, p.relu, p.mask_slot, p.kind, p.chunk_base, 0};
        memcpy(&pass[(size_t)i * 8], o, sizeof o);
    }
    const int32_t meta[9] = {pn.n_fwd, pn.n_pass_all, pn.chunks_fwd, pn.chunks_all, pn.n_bias_rows, pn.wlast_row, pn.w0_row, pn.lat_tile, pn.code_len};
    line("fp32.stream", pn.stream.data(), pn.stream.size() * 4);
    line("fp32.bias", pn.bias.data(), pn.bias.size() * 4);
    line("fp32.pass", pass.data(), pass.size() * 4);
    line("fp32.meta", meta, sizeof meta);
    line("fp32.b_last", &pn.b_last, 4);
    {   // the layouts dsp_create derives from the stream, as dsp_debug_split_layout / dsp_debug_cluster_stream / dsp_debug_code_bias return them
        int32_t l12[12], l32[32];      // off | len | len_fwd, and off | len
        const std::vector<int> order = split_chunk_order(pn, l12, l12 + 4, l12 + 8);
        const std::vector<float> cs = cluster_stream(pn, l32, l32 + 16);
        line("split.layout", l12, sizeof l12);
        line("split.order", order.data(), order.size() * 4);
        line("cluster.layout", l32, sizeof l32);
        line("cluster.stream", cs.data(), cs.size() * 4);
        std::vector<float> code(CODE_LEN, 0.f), cb(2 * WIDTH);
        for (int c = 0; c < code_len; ++c) code[c] = net.w[0][c];
        code_bias_host(pn.codew, pn.b0, pn.blat, code.data(), cb.data());
        line("code_bias", cb.data(), cb.size() * 4);
    }
    for (int bf = 0; bf < 2; ++bf) {
        PackedLp pl;
        const bool ok = pack_decoder_lp_host(&pl, &net.desc, bf != 0);
        lp_lines(bf ? "lp_bf16" : "lp_f16", ok, pl, {pl.n_pass, pl.chunks});
    }
    for (int bf = 0; bf < 2; ++bf) {
        PackedLp pl;
        const bool ok = pack_decoder_lpj_host(&pl, &net.desc, bf != 0);
        lp_lines(bf ? "lpj_bf16" : "lpj_f16", ok, pl, {pl.n_pass, pl.chunks, (WIDTH - code_len - 3) / 16});
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "pack")) return pack(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), (uint32_t)strtoul(argv[6], nullptr, 10));
    if (argc >= 3 && !strcmp(argv[1], "hash")) {
        for (int i = 2; i < argc; ++i) {
            FILE* f = fopen(argv[i], "rb");
            if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
            std::vector<unsigned char> buf((size_t)1 << 20);
            uint64_t h = 0xcbf29ce484222325ull;
            for (size_t n; (n = fread(buf.data(), 1, buf.size(), f)) > 0;) h = fnv1a(buf.data(), n, h);
            fclose(f);
            printf("%016llx\n", (unsigned long long)h);
        }
        return 0;
    }
    fprintf(stderr, "usage: pack_driver pack HIDDEN LATENT_IN CODE_LEN WIDTH SEED | pack_driver hash FILE...\n");
    return 2;
}
