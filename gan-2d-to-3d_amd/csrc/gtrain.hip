// gtrain.hip — the kernels of generator training (gan2shape_amd/gtrain.py, op/conv2d_gradfix.py): the weight gradient
// of the modulated convolution, the heads of the two generator losses (stylegan2-pytorch/train.py:81-100) and the
// exponential moving average of the generator's parameters (train.py:50-55).  All float32.
//
// Modulated weight gradient.  The modulated convolution is y = demod[b,o] * conv(s[b,i] * x, w), so
//     dw[a][g,ky,kx] = sum_{b,p} sa[b,a] A[b,a,p] * sg[b,g] G[b,g,shift(p)]
// with (A, sa, G, sg) = (gy, demod, x, s) or, for the adjoint node and UP2, the pairs swapped.  It is the pixel-
// reduction GEMM of conv_wgrad_core.h with the per-sample scale multiplied at operand load: x * s and gy * demod are
// never written to memory.  Summation order and the split over workgroups are wgrad_plan's: fixed order in one
// workgroup in deterministic mode, float atomics between pixel slices otherwise.
//
// The heads are one workgroup each, in the manner of g2s_d_logistic (dtrain.hip): wave butterfly, then the waves in
// index order, no atomics.  The running path-length mean is read from device memory, so a step reads nothing back.
#include "conv_wgrad_core.h"
#include "wave_sum.h"

namespace g2s {

__global__ __launch_bounds__(WG_THREADS) void modconv_wgrad_kernel(WgradParams p, const float *__restrict__ sa,
                                                                   const float *__restrict__ sg) {
    __shared__ float As[WG_BK][WG_BM + 1];
    __shared__ float Bs[WG_BK][WG_BN + 1];
    wgrad_block<true>(p, As, Bs, blockIdx.x, blockIdx.y, blockIdx.z, sa, sg);
}

// ---------------------------------------------------------------------------------------------- loss heads
constexpr int GH_THREADS = 1024;
constexpr int GH_MAXB = 1024;   // samples of one path-penalty launch: their lengths stay in LDS

// Sum over the workgroup, in every thread: butterfly inside a wave, then the waves in index order.
template <int THREADS> __device__ __forceinline__ float gh_block_sum(float v, float *sm) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
    for (int k = 0; k < THREADS / 64; k++) t += sm[k];
    __syncthreads();
    return t;
}

__device__ __forceinline__ float gh_softplus(float v) { return fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v))); }
__device__ __forceinline__ float gh_sigmoid(float v) {
    const float e = expf(-fabsf(v));
    return v >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// One workgroup.  grad [B, n] with n = L * D.
//     len[b] = sqrt(sum_i grad[b,i]^2 / L),  pm = m0 + decay * (mean len - m0),  pen = mean_b (len[b] - pm)^2
//     d pen / d len[b] = (2 / B) * ((len[b] - pm) - decay * mean_j (len[j] - pm))      (pm is not detached)
//     d pen / d grad[b,i] = d pen / d len[b] * grad[b,i] / (L * len[b])                 (0 where len[b] = 0)
__global__ __launch_bounds__(GH_THREADS) void path_penalty(const float *__restrict__ grad,
                                                           const float *__restrict__ mean_path, float decay,
                                                           float *__restrict__ lengths, float *__restrict__ stats,
                                                           float *__restrict__ dgrad, int B, int L, long n) {
    __shared__ float sm[GH_THREADS / 64];
    __shared__ float len[GH_MAXB], coef[GH_MAXB];
    for (int b = 0; b < B; b++) {
        const float *row = grad + (long)b * n;
        float acc = 0.0f;
        for (long i = threadIdx.x; i < n; i += GH_THREADS) acc += row[i] * row[i];
        acc = gh_block_sum<GH_THREADS>(acc, sm);
        if (threadIdx.x == 0) len[b] = sqrtf(acc / (float)L);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float mean = 0.0f;
        for (int b = 0; b < B; b++) mean += len[b];
        mean /= (float)B;
        const float m0 = mean_path[0];
        const float pm = m0 + decay * (mean - m0);
        float pen = 0.0f, dev = 0.0f;
        for (int b = 0; b < B; b++) {
            const float d = len[b] - pm;
            pen += d * d;
            dev += d;
        }
        dev /= (float)B;
        for (int b = 0; b < B; b++) {
            const float dl = (2.0f / (float)B) * ((len[b] - pm) - decay * dev);
            coef[b] = len[b] > 0.0f ? dl / ((float)L * len[b]) : 0.0f;
        }
        stats[0] = pen / (float)B;
        stats[1] = pm;
        stats[2] = mean;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += GH_THREADS) lengths[b] = len[b];
    if (dgrad) {
        for (int b = 0; b < B; b++) {
            const float c = coef[b];
            const long at = (long)b * n;
            for (long i = threadIdx.x; i < n; i += GH_THREADS) dgrad[at + i] = c * grad[at + i];
        }
    }
}

// One workgroup.  out[0] = mean softplus(-fake); g_fake [B] = -sigmoid(-fake) / B (optional).
__global__ __launch_bounds__(256) void g_nonsaturating(const float *__restrict__ fake, float *__restrict__ out,
                                                       float *__restrict__ g_fake, int B) {
    __shared__ float sm[256 / 64];
    float l = 0.0f;
    for (int i = threadIdx.x; i < B; i += 256) {
        const float v = fake[i];
        l += gh_softplus(-v);
        if (g_fake) g_fake[i] = -gh_sigmoid(-v) / (float)B;
    }
    l = gh_block_sum<256>(l, sm);
    if (threadIdx.x == 0) out[0] = l / (float)B;
}

// ------------------------------------------------------------------------------------------------------ EMA
typedef float em_v4 __attribute__((ext_vector_type(4)));
constexpr int EM_THREADS = 256;
constexpr int EM_CHUNK = 256 * 4 * 8;   // elements per block: 8 lanes of 16 bytes per thread

// dst = dst * decay + src * (1 - decay) over a device table of tensors; a block finds its tensor by bisection over
// the chunk prefix and updates one chunk.  Streaming: 8 bytes read and 4 written per element.
__global__ __launch_bounds__(EM_THREADS) void ema_accumulate(const g2s_ema_tensor *__restrict__ tensors,
                                                             const int *__restrict__ chunk0, int n_tensors, float decay,
                                                             float rest) {
    int lo = 0, hi = n_tensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk0[mid] <= (int)blockIdx.x) lo = mid;
        else hi = mid;
    }
    const g2s_ema_tensor t = tensors[lo];
    const int64_t base = (int64_t)(blockIdx.x - chunk0[lo]) * EM_CHUNK;
    const bool vec = ((reinterpret_cast<uintptr_t>(t.dst) | reinterpret_cast<uintptr_t>(t.src)) & 15) == 0;
#pragma unroll
    for (int it = 0; it < 8; it += 4) {
        int64_t idx[4];
        em_v4 d[4], s[4];
        bool full[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {   // the loads of a trip before its first store
            idx[u] = base + ((int64_t)(it + u) * EM_THREADS + threadIdx.x) * 4;
            full[u] = vec && idx[u] + 4 <= t.n;
            if (full[u]) {
                d[u] = *reinterpret_cast<const em_v4 *>(t.dst + idx[u]);
                s[u] = __builtin_nontemporal_load(reinterpret_cast<const em_v4 *>(t.src + idx[u]));
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (full[u]) {
                *reinterpret_cast<em_v4 *>(t.dst + idx[u]) = d[u] * decay + s[u] * rest;
            } else {
                for (int64_t j = idx[u]; j < idx[u] + 4 && j < t.n; j++) t.dst[j] = t.dst[j] * decay + t.src[j] * rest;
            }
        }
    }
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_modconv_wgrad(const float *A, const float *sa, const float *G, const float *sg, float *dw, int B,
                                 int Ca, int Cg, int PH, int PW, int GH, int GW, int k, int stride, int pad,
                                 int dw_is_zero, g2s_stream_t stream) {
    WgradParams p;
    int tiles, split;
    const int rc = wgrad_plan(A, G, dw, B, Ca, Cg, PH, PW, GH, GW, k, stride, pad, 1, p, tiles, split);
    if (rc != G2S_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (p.atomic && !dw_is_zero && hipMemsetAsync(dw, 0, (size_t)Ca * p.N * sizeof(float), st) != hipSuccess)
        return fail(G2S_ERR_LAUNCH, "hipMemsetAsync(dw) failed");
    modconv_wgrad_kernel<<<dim3(tiles, split, 1), WG_THREADS, 0, st>>>(p, sa, sg);
    return check_launch("g2s_modconv_wgrad");
}

extern "C" int g2s_path_penalty(const float *grad, const float *mean_path, float decay, float *lengths, float *stats,
                                float *dgrad, int B, int L, int D, g2s_stream_t stream) {
    G2S_REQUIRE(grad && mean_path && lengths && stats, "g2s_path_penalty: NULL pointer argument");
    G2S_REQUIRE(B > 0 && B <= GH_MAXB && L > 0 && D > 0, "g2s_path_penalty: 1 <= B <= %d, L and D positive", GH_MAXB);
    G2S_REQUIRE((long)B * L * D < (1l << 31), "g2s_path_penalty: tensor too large");
    path_penalty<<<1, GH_THREADS, 0, as_stream(stream)>>>(grad, mean_path, decay, lengths, stats, dgrad, B, L,
                                                          (long)L * D);
    return check_launch("g2s_path_penalty");
}

extern "C" int g2s_g_nonsaturating(const float *fake, float *out, float *g_fake, int B, g2s_stream_t stream) {
    G2S_REQUIRE(fake && out && B > 0, "g2s_g_nonsaturating: NULL pointer or empty batch");
    g_nonsaturating<<<1, 256, 0, as_stream(stream)>>>(fake, out, g_fake, B);
    return check_launch("g2s_g_nonsaturating");
}

extern "C" int64_t g2s_ema_chunk(void) { return EM_CHUNK; }

extern "C" int g2s_ema_accumulate(const g2s_ema_tensor *tensors, const int *chunk0, int n_tensors, int n_chunks,
                                  float decay, float one_minus_decay, g2s_stream_t stream) {
    G2S_REQUIRE(tensors && chunk0, "g2s_ema_accumulate: NULL pointer argument");
    G2S_REQUIRE(n_tensors > 0 && n_chunks >= n_tensors, "g2s_ema_accumulate: a chunk per tensor at least");
    ema_accumulate<<<n_chunks, EM_THREADS, 0, as_stream(stream)>>>(tensors, chunk0, n_tensors, decay, one_minus_decay);
    return check_launch("g2s_ema_accumulate");
}
