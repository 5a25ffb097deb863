// dtrain.hip — the small kernels of discriminator training (gan2shape_amd/dtrain.py): the minibatch-stddev feature
// of the discriminator's last block with its backward and double backward, the logistic loss head and the R1
// penalty (stylegan2-pytorch/model.py:756-765, train.py:64-78).  Every tensor here is a few KB to a few MB: the
// cost is launches and latency, not bandwidth, so each entry is one launch (the R1 penalty: two stages), float32,
// with a fixed summation order (wave butterfly, then the waves in index order) and no atomics — results repeat bit
// for bit.
//
// Minibatch stddev.  x [B, C, H, W], G = min(B, 4) members per group, M = B / G groups, F feature blocks of
// C / F channels, E = (C / F) * H * W elements per block.  Member g of group n is sample g * M + n.
//     d_g = x_g - mean_g x,   s = sqrt(mean_g d_g^2 + eps),   f[n, j] = mean_e s
// One workgroup per (group n, block j) walks the E elements: the G values of an element are G loads of one thread,
// so mean, d and s never leave registers; the block's sum of s is the workgroup's reduction.
#include "g2s_common.h"
#include "wave_sum.h"

namespace g2s {

constexpr int MB_THREADS = 1024;
constexpr int MB_MAXG = 4;
constexpr float MB_EPS = 1e-8f;
// the members of a group: unrolled to the most a group holds, so that their values stay in registers
#define MB_EACH_MEMBER(g) _Pragma("unroll") for (int g = 0; g < MB_MAXG; g++) if (g < q.G)

// Sum over the workgroup, in every thread: butterfly inside a wave, then the waves in index order.  `sm` holds one
// float per wave; two barriers, so the same `sm` can serve the next call.
template <int THREADS> __device__ __forceinline__ float block_sum(float v, float *sm) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
    for (int k = 0; k < THREADS / 64; k++) t += sm[k];
    __syncthreads();
    return t;
}

struct MbGeom {
    int B, C, HW, G, M, F, E;   // E = (C / F) * HW
};

// offset of element e of block j in sample b of a [*, Ctot, HW] tensor
__device__ __forceinline__ long mb_at(const MbGeom &q, int b, int j, int e, int Ctot) {
    return ((long)b * Ctot + (long)j * (q.C / q.F)) * q.HW + e;
}

// mean-free values and s of one element: d[g] for g < G, returns s
__device__ __forceinline__ float mb_stats(const MbGeom &q, const float *__restrict__ x, int n, int j, int e, float *d) {
    float mean = 0.0f;
    MB_EACH_MEMBER(g) {
        d[g] = x[mb_at(q, g * q.M + n, j, e, q.C)];
        mean += d[g];
    }
    mean /= (float)q.G;
    float var = 0.0f;
    MB_EACH_MEMBER(g) {
        d[g] -= mean;
        var += d[g] * d[g];
    }
    return sqrtf(var / (float)q.G + MB_EPS);
}

// grid (M, F).  out [B, C + F, HW]: the copy of x and the F constant maps.
__global__ __launch_bounds__(MB_THREADS) void mbstd_fwd(const float *__restrict__ x, float *__restrict__ out, MbGeom q) {
    __shared__ float sm[MB_THREADS / 64];
    const int n = blockIdx.x, j = blockIdx.y, Ct = q.C + q.F;
    float acc = 0.0f, d[MB_MAXG];
    for (int e = threadIdx.x; e < q.E; e += MB_THREADS) {
        float mean = 0.0f;
        MB_EACH_MEMBER(g) {
            const int b = g * q.M + n;
            d[g] = x[mb_at(q, b, j, e, q.C)];
            out[mb_at(q, b, j, e, Ct)] = d[g];
            mean += d[g];
        }
        mean /= (float)q.G;
        float var = 0.0f;
        MB_EACH_MEMBER(g) {
            const float t = d[g] - mean;
            var += t * t;
        }
        acc += sqrtf(var / (float)q.G + MB_EPS);
    }
    const float f = block_sum<MB_THREADS>(acc, sm) / (float)q.E;
    for (int i = threadIdx.x; i < q.G * q.HW; i += MB_THREADS) {
        const int b = (i / q.HW) * q.M + n;
        out[((long)b * Ct + q.C + j) * q.HW + i % q.HW] = f;
    }
}

// sum of the appended map j over the members of group n: gf[n, j]
template <int THREADS>
__device__ __forceinline__ float mb_map_sum(const MbGeom &q, const float *__restrict__ gout, int n, int j, float *sm) {
    float acc = 0.0f;
    for (int i = threadIdx.x; i < q.G * q.HW; i += THREADS) {
        const int b = (i / q.HW) * q.M + n;
        acc += gout[((long)b * (q.C + q.F) + q.C + j) * q.HW + i % q.HW];
    }
    return block_sum<THREADS>(acc, sm);
}

// grid (M, F).  gx = gout[:, :C] + a * d / s,  a = gf / (E * G).
__global__ __launch_bounds__(MB_THREADS) void mbstd_bwd(const float *__restrict__ gout, const float *__restrict__ x,
                                                        float *__restrict__ gx, MbGeom q) {
    __shared__ float sm[MB_THREADS / 64];
    const int n = blockIdx.x, j = blockIdx.y, Ct = q.C + q.F;
    const float a = mb_map_sum<MB_THREADS>(q, gout, n, j, sm) / ((float)q.E * (float)q.G);
    float d[MB_MAXG];
    for (int e = threadIdx.x; e < q.E; e += MB_THREADS) {
        const float r = a / mb_stats(q, x, n, j, e, d);
        MB_EACH_MEMBER(g) {
            const int b = g * q.M + n;
            gx[mb_at(q, b, j, e, q.C)] = gout[mb_at(q, b, j, e, Ct)] + r * d[g];
        }
    }
}

// grid (M, F).  The backward of mbstd_bwd for a cotangent ggx on gx:
//     ggout[:, :C] = ggx,   ggout[:, C + j] = T = sum_{g,e} ggx_g d_g / (s E G)   on every member of the group
//     xg_h = a * [ (ggx_h - mean_g ggx) / s - d_h * (sum_g ggx_g d_g) / (G s^3) ]
__global__ __launch_bounds__(MB_THREADS) void mbstd_bwd2(const float *__restrict__ ggx, const float *__restrict__ gout,
                                                         const float *__restrict__ x, float *__restrict__ ggout,
                                                         float *__restrict__ xg, MbGeom q) {
    __shared__ float sm[MB_THREADS / 64];
    const int n = blockIdx.x, j = blockIdx.y, Ct = q.C + q.F;
    const float a = mb_map_sum<MB_THREADS>(q, gout, n, j, sm) / ((float)q.E * (float)q.G);
    float acc = 0.0f, d[MB_MAXG], u[MB_MAXG];
    for (int e = threadIdx.x; e < q.E; e += MB_THREADS) {
        const float s = mb_stats(q, x, n, j, e, d);
        float um = 0.0f, ud = 0.0f;
        MB_EACH_MEMBER(g) {
            const int b = g * q.M + n;
            u[g] = ggx[mb_at(q, b, j, e, q.C)];
            ggout[mb_at(q, b, j, e, Ct)] = u[g];
            um += u[g];
            ud += u[g] * d[g];
        }
        um /= (float)q.G;
        const float rs = 1.0f / s, c = ud * rs * rs * rs / (float)q.G;
        acc += ud * rs;
        MB_EACH_MEMBER(g)
            xg[mb_at(q, g * q.M + n, j, e, q.C)] = a * ((u[g] - um) * rs - d[g] * c);
    }
    const float T = block_sum<MB_THREADS>(acc, sm) / ((float)q.E * (float)q.G);
    for (int i = threadIdx.x; i < q.G * q.HW; i += MB_THREADS) {
        const int b = (i / q.HW) * q.M + n;
        ggout[((long)b * Ct + q.C + j) * q.HW + i % q.HW] = T;
    }
}

// ---------------------------------------------------------------------------------------------- loss heads
constexpr int LH_THREADS = 256;

__device__ __forceinline__ float softplus(float v) { return fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v))); }
// 1 / (1 + exp(-v)) without overflow for either sign
__device__ __forceinline__ float sigmoid(float v) {
    const float e = expf(-fabsf(v));
    return v >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// One workgroup.  out[0] = mean softplus(-real) + mean softplus(fake), out[1] = mean real, out[2] = mean fake,
// out[3] = sum sign(real); g_real = -sigmoid(-real) / Br, g_fake = sigmoid(fake) / Bf (both optional).
__global__ __launch_bounds__(LH_THREADS) void d_logistic(const float *__restrict__ real, const float *__restrict__ fake,
                                                         float *__restrict__ out, float *__restrict__ g_real,
                                                         float *__restrict__ g_fake, int Br, int Bf) {
    __shared__ float sm[LH_THREADS / 64];
    float lr = 0.0f, lf = 0.0f, mr = 0.0f, mf = 0.0f, sg = 0.0f;
    for (int i = threadIdx.x; i < Br; i += LH_THREADS) {
        const float v = real[i];
        lr += softplus(-v);
        mr += v;
        sg += v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f);
        if (g_real) g_real[i] = -sigmoid(-v) / (float)Br;
    }
    for (int i = threadIdx.x; i < Bf; i += LH_THREADS) {
        const float v = fake[i];
        lf += softplus(v);
        mf += v;
        if (g_fake) g_fake[i] = sigmoid(v) / (float)Bf;
    }
    lr = block_sum<LH_THREADS>(lr, sm);
    lf = block_sum<LH_THREADS>(lf, sm);
    mr = block_sum<LH_THREADS>(mr, sm);
    mf = block_sum<LH_THREADS>(mf, sm);
    sg = block_sum<LH_THREADS>(sg, sm);
    if (threadIdx.x == 0) {
        out[0] = lr / (float)Br + lf / (float)Bf;
        out[1] = mr / (float)Br;
        out[2] = mf / (float)Bf;
        out[3] = sg;
    }
}

constexpr int R1_CHUNK = 4096;   // floats of one sample that one workgroup of the first stage squares and adds

// stage 1, grid (chunks, B): partial[b, chunk] = sum of squares of the chunk
__global__ __launch_bounds__(LH_THREADS) void r1_partial(const float *__restrict__ grad, float *__restrict__ partial,
                                                         long n, int chunks) {
    __shared__ float sm[LH_THREADS / 64];
    const float *row = grad + (long)blockIdx.y * n;
    const long lo = (long)blockIdx.x * R1_CHUNK, hi = lo + R1_CHUNK < n ? lo + R1_CHUNK : n;
    float acc = 0.0f;
    for (long i = lo + threadIdx.x; i < hi; i += LH_THREADS) acc += row[i] * row[i];
    acc = block_sum<LH_THREADS>(acc, sm);
    if (threadIdx.x == 0) partial[(long)blockIdx.y * chunks + blockIdx.x] = acc;
}

// stage 2, one workgroup: per_sample[b] = the chunks of b in index order; mean[0] = their mean over b, in index order
__global__ __launch_bounds__(LH_THREADS) void r1_finish(const float *__restrict__ partial, float *__restrict__ per_sample,
                                                        float *__restrict__ mean, int B, int chunks) {
    for (int b = threadIdx.x; b < B; b += LH_THREADS) {
        float acc = 0.0f;
        for (int c = 0; c < chunks; c++) acc += partial[(long)b * chunks + c];
        per_sample[b] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0 && mean) {
        float acc = 0.0f;
        for (int b = 0; b < B; b++) acc += per_sample[b];
        mean[0] = acc / (float)B;
    }
}

}  // namespace g2s

using namespace g2s;

static int mb_geom(const char *who, int B, int C, int H, int W, int F, MbGeom &q) {
    G2S_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && F > 0, "%s: sizes must be positive", who);
    const int G = B < MB_MAXG ? B : MB_MAXG;
    G2S_REQUIRE(B % G == 0, "%s: batch %d is no multiple of the group size %d", who, B, G);
    G2S_REQUIRE(C % F == 0, "%s: %d channels do not split into %d feature blocks", who, C, F);
    G2S_REQUIRE((long)B * (C + F) * H * W < (1l << 31) && B / G <= 65535 && F <= 65535, "%s: tensor too large", who);
    q = MbGeom{B, C, H * W, G, B / G, F, (C / F) * H * W};
    return G2S_OK;
}

extern "C" int g2s_mbstd_fwd(const float *x, float *out, int B, int C, int H, int W, int F, g2s_stream_t stream) {
    G2S_REQUIRE(x && out, "g2s_mbstd_fwd: NULL pointer argument");
    MbGeom q;
    const int rc = mb_geom("g2s_mbstd_fwd", B, C, H, W, F, q);
    if (rc != G2S_OK) return rc;
    mbstd_fwd<<<dim3(q.M, q.F), MB_THREADS, 0, as_stream(stream)>>>(x, out, q);
    return check_launch("g2s_mbstd_fwd");
}

extern "C" int g2s_mbstd_bwd(const float *gout, const float *x, float *gx, int B, int C, int H, int W, int F,
                             g2s_stream_t stream) {
    G2S_REQUIRE(gout && x && gx, "g2s_mbstd_bwd: NULL pointer argument");
    MbGeom q;
    const int rc = mb_geom("g2s_mbstd_bwd", B, C, H, W, F, q);
    if (rc != G2S_OK) return rc;
    mbstd_bwd<<<dim3(q.M, q.F), MB_THREADS, 0, as_stream(stream)>>>(gout, x, gx, q);
    return check_launch("g2s_mbstd_bwd");
}

extern "C" int g2s_mbstd_bwd2(const float *ggx, const float *gout, const float *x, float *ggout, float *xg, int B, int C,
                              int H, int W, int F, g2s_stream_t stream) {
    G2S_REQUIRE(ggx && gout && x && ggout && xg, "g2s_mbstd_bwd2: NULL pointer argument");
    MbGeom q;
    const int rc = mb_geom("g2s_mbstd_bwd2", B, C, H, W, F, q);
    if (rc != G2S_OK) return rc;
    mbstd_bwd2<<<dim3(q.M, q.F), MB_THREADS, 0, as_stream(stream)>>>(ggx, gout, x, ggout, xg, q);
    return check_launch("g2s_mbstd_bwd2");
}

extern "C" int g2s_d_logistic(const float *real, const float *fake, float *out, float *g_real, float *g_fake, int Br,
                              int Bf, g2s_stream_t stream) {
    G2S_REQUIRE(real && fake && out && Br > 0 && Bf > 0, "g2s_d_logistic: NULL pointer or empty batch");
    d_logistic<<<1, LH_THREADS, 0, as_stream(stream)>>>(real, fake, out, g_real, g_fake, Br, Bf);
    return check_launch("g2s_d_logistic");
}

extern "C" int64_t g2s_r1_penalty_chunks(int64_t n) { return n > 0 ? (n + R1_CHUNK - 1) / R1_CHUNK : 0; }

extern "C" int g2s_r1_penalty(const float *grad, float *per_sample, float *mean, float *partial, int B, int64_t n,
                              g2s_stream_t stream) {
    G2S_REQUIRE(grad && per_sample && partial && B > 0 && n > 0, "g2s_r1_penalty: NULL pointer or empty tensor");
    const int64_t chunks = g2s_r1_penalty_chunks(n);
    G2S_REQUIRE(B <= 65535 && chunks < (1l << 31), "g2s_r1_penalty: tensor too large");
    r1_partial<<<dim3((unsigned)chunks, B), LH_THREADS, 0, as_stream(stream)>>>(grad, partial, (long)n, (int)chunks);
    r1_finish<<<1, LH_THREADS, 0, as_stream(stream)>>>(partial, per_sample, mean, B, (int)chunks);
    return check_launch("g2s_r1_penalty");
}
