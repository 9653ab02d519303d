// What the other host files call in decoder_calls.hip: the decoder's upload and calibration at dsp_create, the argument blocks of the decoder
// launches, the device-resident single-shot decode and the host copy of the margin table's read-out.
#pragma once
#include "host_common.h"

namespace dsp_host __attribute__((visibility("hidden"))) {      // (the attribute covers this block only: without it these seven would be exports)

void pack_decoder(dsp_handle* h, const dsp_decoder_desc* d);
LpjArgs make_lpj_args(const dsp_handle* h, bool bf, int which);
LpArgs make_lp_args(const dsp_handle* h, bool bf);
MlpArgs make_mlp_args(const dsp_handle* h, int mode);
void decode_resident_points(dsp_handle* h, const float* codes, int64_t n_codes, int64_t n, bool bwd, int lp = 0, float* out = nullptr);
void calibrate_prepass(dsp_handle* h);
float lp_delta_host(const float* code, const LpDeltaTab& t);

}  // namespace dsp_host
