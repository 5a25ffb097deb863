// synth_batch.hip — the frozen generator with ONE NOISE MAP PER SAMPLE (synthesis.py under per_sample_noise: the
// batched latent projector and the batched sampler).
//
//   g2s_noise_bias_act_ps   y[b,c,i] = gain * lrelu(x[b,c,i] + noise_w[0] * noise[b,i] + bias[c], alpha): the StyledConv
//                           tail (stylegan2-pytorch/model.py:349-355) behind a convolution that ran with its scales
//                           only.  HBM-bound, 2 x B x C x HW x 4 bytes (the maps are C times smaller and stay in L2);
//                           16 bytes per lane per access, one (b, c) row per blockIdx.y.  The additions are those of
//                           g2s_noise_bias_act (fused_bias_act.hip) in its order and under the same contraction
//                           setting: equal maps give its bits.
//
// Its siblings share a kernel template with the shared-map entries: g2s_upfirdn2d_nba_ps in upfirdn2d.hip,
// g2s_synth_bwd_rows_ps in rowops.hip.
#include <algorithm>
#include "g2s_common.h"

namespace g2s {

__device__ __forceinline__ float lrelu_gain(float x, float alpha, float scale) {
    const float y = (x > 0.0f) ? x : x * alpha;
    return y * scale;
}

// grid (ceil(HW4 / 256) capped at 64, B * C); x and y may be the same buffer
__global__ __launch_bounds__(256) void noise_bias_act_ps_vec4(const float4 *x, const float4 *__restrict__ noise,
                                                              const float *__restrict__ noise_w,
                                                              const float *__restrict__ bias, float4 *y, int C, int HW4,
                                                              float alpha, float scale) {
    const int row = blockIdx.y;
    const float bb = bias ? bias[row % C] : 0.0f;
    const float nw = noise_w[0];
    const float4 *xr = x + (size_t)row * HW4;
    const float4 *nr = noise + (size_t)(row / C) * HW4;
    float4 *yr = y + (size_t)row * HW4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW4; i += gridDim.x * blockDim.x) {
        float4 v = xr[i];
        const float4 nz = nr[i];
        v.x += nw * nz.x;
        v.y += nw * nz.y;
        v.z += nw * nz.z;
        v.w += nw * nz.w;
        float4 o;
        o.x = lrelu_gain(v.x + bb, alpha, scale);
        o.y = lrelu_gain(v.y + bb, alpha, scale);
        o.z = lrelu_gain(v.z + bb, alpha, scale);
        o.w = lrelu_gain(v.w + bb, alpha, scale);
        yr[i] = o;
    }
}

__global__ __launch_bounds__(256) void noise_bias_act_ps_scalar(const float *x, const float *__restrict__ noise,
                                                                const float *__restrict__ noise_w,
                                                                const float *__restrict__ bias, float *y, int C, int HW,
                                                                float alpha, float scale) {
    const int row = blockIdx.y;
    const float bb = bias ? bias[row % C] : 0.0f;
    const float nw = noise_w[0];
    const float *nr = noise + (size_t)(row / C) * HW;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
        float v = x[(size_t)row * HW + i];
        v += nw * nr[i];
        y[(size_t)row * HW + i] = lrelu_gain(v + bb, alpha, scale);
    }
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_noise_bias_act_ps(const float *x, const float *noise, const float *noise_w, const float *bias,
                                     float *y, int B, int C, int HW, float alpha, float scale, g2s_stream_t stream) {
    G2S_REQUIRE(x && y && noise && noise_w, "g2s_noise_bias_act_ps: x, y, noise, noise_w must not be NULL");
    G2S_REQUIRE(B > 0 && C > 0 && HW > 0, "g2s_noise_bias_act_ps: B, C, HW must be positive");
    G2S_REQUIRE((long)B * C <= 65535, "g2s_noise_bias_act_ps: B*C too large for grid.y");
    hipStream_t st = as_stream(stream);
    const uintptr_t bits = (uintptr_t)x | (uintptr_t)y | (uintptr_t)noise;
    if (HW % 4 == 0 && (bits & 15) == 0) {
        const int HW4 = HW / 4;
        noise_bias_act_ps_vec4<<<dim3(std::min(cdiv(HW4, 256), 64), B * C), 256, 0, st>>>(
            (const float4 *)x, (const float4 *)noise, noise_w, bias, (float4 *)y, C, HW4, alpha, scale);
    } else {
        noise_bias_act_ps_scalar<<<dim3(std::min(cdiv(HW, 256), 64), B * C), 256, 0, st>>>(x, noise, noise_w, bias, y, C,
                                                                                            HW, alpha, scale);
    }
    return check_launch("g2s_noise_bias_act_ps");
}
