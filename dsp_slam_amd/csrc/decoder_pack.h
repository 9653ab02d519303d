// Decoder packing: weights -> the weight streams the decoder kernels read, in MFMA operand order (mlp_kernel.hip / DESIGN.md).
// Pure host arithmetic: no handle, no HIP runtime call, so it also builds into a stand-alone program (tests/host/pack_driver.cpp).
#pragma once
#include "dsp_gn.h"
#include "dsp_internal.h"

#include <vector>

namespace dsp_host __attribute__((visibility("hidden"))) {
using namespace dsp;

struct PackedNet {
    std::vector<float> stream, bias;
    std::vector<float> codew;   // [2][512][64]: W0[:, :64] and W_lat[:, code columns], row-major
    std::vector<float> b0, blat;
    float b_last = 0.f;
    int wlast_row = 0, w0_row = 0;
    int n_bias_rows = 0, n_fwd = 0, n_pass_all = 0, chunks_fwd = 0, chunks_all = 0;
    int lat_tile = 27, code_len = CODE_LEN;   // 16-row slab tile holding the re-injected xyz (27: rows 445..447, 29: 477..479)
    PassDesc pass[MAX_PASSES];
};

struct PackedLp {
    std::vector<uint16_t> stream;
    LpPass pass[LP_MAX_PASSES];
    int n_pass = 0, chunks = 0;
};

void pack_decoder_host(PackedNet* h, const dsp_decoder_desc* d);
bool pack_decoder_lp_host(PackedLp* out, const dsp_decoder_desc* d, bool bf);
bool pack_decoder_lpj_host(PackedLp* out, const dsp_decoder_desc* d, bool bf);
std::vector<int> split_chunk_order(const PackedNet& pn, int off[4], int len[4], int len_fwd[4]);
std::vector<float> cluster_stream(const PackedNet& pn, int off[16], int len[16]);
void code_bias_host(const std::vector<float>& codew, const std::vector<float>& b0, const std::vector<float>& blat, const float* code,
                    float* out /*1024*/);

}  // namespace dsp_host
