// mapping.hip — the sample generator's kernels (generate.py): the mapping network in one launch, the ordered mean of
// the truncation latent, and the image quantiser.  No backward: nothing here carries a gradient.
//
//   mapping_kernel<NTW>   PixelNorm + L x (EqualLinear + bias + leaky ReLU * gain) + truncation lerp for one tile of
//                         MAP_T = 16 rows.  One workgroup of 4 waves owns the tile through all layers.  The tile's
//                         activation h [16][D + 4] lives in LDS (33 KB at D = 512; the pad of 4 floats spreads the 16
//                         rows of a 128-bit fragment read over all banks) and is updated IN PLACE: a layer's D x 16
//                         outputs are complete in the accumulators (wave w owns the 16-column tiles w, w + 4, ...,
//                         NTW <= 8 of them, 4 VGPRs each) before a barrier lets them overwrite h.
//                         Products are v_mfma_f32_16x16x4_f32 (exact f32, an fmaf chain along K).  Per chunk of 32 K a
//                         lane (i = lane & 15, q = lane >> 4) holds 8 consecutive K values of row i of the A tile
//                         (from LDS) and of weight row i of each of its B tiles (from global memory: 16 rows x 128
//                         contiguous bytes per tile, two 16-byte loads per lane), k = 32 c + 8 q + e for e = 0..7;
//                         MFMA e of the chunk pairs element e of both, so every k meets its own partner — the order
//                         of K inside the sum is a permutation, nothing else.  The weight registers of chunk c + 1 are
//                         loaded while chunk c multiplies.  Weights are not staged in LDS: every byte of a layer is
//                         used by exactly one wave of the workgroup, L2 is the shared level (the whole stack is 8 MB).
//                         What bounds it: 16 rows give 8 FLOP per weight byte, i.e. 32 B/clk/CU of L2 reads at the
//                         full MFMA rate; 16 rows is what fills 256 CUs at N = 4096.  Measured the
//                         launch is latency bound: 2.1 us per chunk against 0.85 us of MFMA issue, flat in N.
//                         Rows past N are zero-filled in LDS, computed and never stored.  No atomics: a tile depends
//                         on nothing outside itself, `partial` row t is tile t's column sums over its valid rows in
//                         ascending row order.
//   rows_mean_kernel      out[d] = (sum over tiles t ascending of partial[t][d]) / N, one thread per column: the
//                         same bits on every run (no atomics, no dependence on g2s_set_deterministic).
//   image_to_u8_kernel<W> [B,3,H,W] f32 -> [B,H,W,3] u8 with the arithmetic of torchvision's
//                         save_image(normalize=True, range=(-1, 1)): clamp(-1, 1), + 1, / 2, * 255, + 0.5, clamp(0, 255),
//                         truncate.  This file is built with -ffp-contract=off, so each step rounds as the torch
//                         expression does.  W = 4: a thread reads one float4 per channel and writes 12 bytes.
#include "g2s_common.h"

namespace g2s {

constexpr int MAP_T = 16;        // rows per tile (g2s_mapping_tile)
constexpr int MAP_DMAX = 512;
constexpr int MAP_PAD = 4;
constexpr int MAP_WAVES = 4;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MapParams {
    const float *z;        // [N, D]
    const float *w;        // [L, D, D]
    const float *b;        // [L, D]
    const float *center;   // [D] or NULL
    float *out;            // [N, D]
    float *partial;        // [tiles, D] or NULL
    long N;
    int D, L, pixel_norm;
    float alpha, gain, truncation;
};

template <int NTW>
__global__ __launch_bounds__(256) void mapping_kernel(MapParams p) {
    __shared__ __attribute__((aligned(16))) float h[MAP_T * (MAP_DMAX + MAP_PAD)];
    const int D = p.D, LD = D + MAP_PAD, D4 = D / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * MAP_T;
    const int nvalid = (int)(p.N - row0 < MAP_T ? p.N - row0 : MAP_T);

    // the tile of z, rows past N as zeros
    for (int i = tid; i < MAP_T * D4; i += 256) {
        const int r = i / D4, c = i - r * D4;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < nvalid) v = *reinterpret_cast<const float4 *>(p.z + (size_t)(row0 + r) * D + c * 4);
        *reinterpret_cast<float4 *>(&h[r * LD + c * 4]) = v;
    }
    __syncthreads();
    if (p.pixel_norm) {   // 16 threads per row; h * rsqrt(mean(h^2) + 1e-8)
        const int r = tid >> 4, s = tid & 15;
        float ss = 0.0f;
        for (int k = s; k < D; k += 16) ss += h[r * LD + k] * h[r * LD + k];
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 16);
        const float scale = 1.0f / sqrtf(ss / (float)D + 1e-8f);
        for (int k = s; k < D; k += 16) h[r * LD + k] *= scale;
        __syncthreads();
    }

    const int CT = D / 16;                 // 16-column tiles of a layer's output
    const int fi = lane & 15, fq = lane >> 4;
    const int nchunk = D / 32;
    for (int l = 0; l < p.L; l++) {
        const float *W = p.w + (size_t)l * D * D;
        const float *wrow[NTW];
#pragma unroll
        for (int t = 0; t < NTW; t++) {
            int ct = wave + MAP_WAVES * t;
            if (ct >= CT) ct = CT - 1;     // a wave without a tile recomputes the last one and stores nothing
            wrow[t] = W + (size_t)(ct * 16 + fi) * D + fq * 8;
        }
        f32x4 acc[NTW];
#pragma unroll
        for (int t = 0; t < NTW; t++) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        float4 bc[NTW][2], bn[NTW][2];
#pragma unroll
        for (int t = 0; t < NTW; t++) {
            bc[t][0] = *reinterpret_cast<const float4 *>(wrow[t]);
            bc[t][1] = *reinterpret_cast<const float4 *>(wrow[t] + 4);
        }
        const float *arow = &h[fi * LD + fq * 8];
        for (int c = 0; c < nchunk; c++) {
            if (c + 1 < nchunk) {
#pragma unroll
                for (int t = 0; t < NTW; t++) {
                    bn[t][0] = *reinterpret_cast<const float4 *>(wrow[t] + (c + 1) * 32);
                    bn[t][1] = *reinterpret_cast<const float4 *>(wrow[t] + (c + 1) * 32 + 4);
                }
            }
            const float4 a0 = *reinterpret_cast<const float4 *>(arow + c * 32);
            const float4 a1 = *reinterpret_cast<const float4 *>(arow + c * 32 + 4);
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int e = 0; e < 8; e++) {
#pragma unroll
                for (int t = 0; t < NTW; t++) {
                    const float4 bq = bc[t][e >> 2];
                    const float bv = (e & 3) == 0 ? bq.x : (e & 3) == 1 ? bq.y : (e & 3) == 2 ? bq.z : bq.w;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bv, acc[t], 0, 0, 0);
                }
            }
            if (c + 1 < nchunk) {
#pragma unroll
                for (int t = 0; t < NTW; t++) {
                    bc[t][0] = bn[t][0];
                    bc[t][1] = bn[t][1];
                }
            }
        }
        __syncthreads();   // every wave has read h for this layer
        // C layout of 16x16x4: column = lane & 15 (output feature), row = 4 * (lane >> 4) + register
#pragma unroll
        for (int t = 0; t < NTW; t++) {
            const int ct = wave + MAP_WAVES * t;
            if (ct < CT) {
                const int col = ct * 16 + fi;
                const float bias = p.b[(size_t)l * D + col];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = acc[t][r] + bias;
                    v = v > 0.0f ? v : v * p.alpha;
                    h[(fq * 4 + r) * LD + col] = v * p.gain;
                }
            }
        }
        __syncthreads();
    }

    if (p.center) {
        for (int i = tid; i < MAP_T * D; i += 256) {
            const int r = i / D, k = i - r * D;
            const float c = p.center[k];
            h[r * LD + k] = c + p.truncation * (h[r * LD + k] - c);
        }
        __syncthreads();
    }
    for (int i = tid; i < nvalid * D4; i += 256) {
        const int r = i / D4, c = i - r * D4;
        *reinterpret_cast<float4 *>(p.out + (size_t)(row0 + r) * D + c * 4) =
            *reinterpret_cast<const float4 *>(&h[r * LD + c * 4]);
    }
    if (p.partial) {
        for (int k = tid; k < D; k += 256) {
            float s = 0.0f;
            for (int r = 0; r < nvalid; r++) s += h[r * LD + k];
            p.partial[(size_t)blockIdx.x * D + k] = s;
        }
    }
}

__global__ __launch_bounds__(256) void rows_mean_kernel(const float *__restrict__ partial, float *__restrict__ out,
                                                        long tiles, int D, float n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= D) return;
    float s = 0.0f;
#pragma unroll 8   // eight loads in flight; the additions keep their order
    for (long t = 0; t < tiles; t++) s += partial[(size_t)t * D + k];
    out[k] = s / n;
}

__device__ __forceinline__ unsigned quantise(float x) {
    x = fminf(fmaxf(x, -1.0f), 1.0f);
    x = (x + 1.0f) / 2.0f;
    x = x * 255.0f + 0.5f;
    x = fminf(fmaxf(x, 0.0f), 255.0f);
    return (unsigned)(int)x;
}

template <int W>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const float *__restrict__ x, uint8_t *__restrict__ out,
                                                          long B, long HW) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * W;   // pixel index within [B, H*W]
    if (i >= B * HW) return;
    const long b = i / HW, s = i - b * HW;
    const float *src = x + (size_t)b * 3 * HW + s;
    if (W == 4) {
        const float4 r = *reinterpret_cast<const float4 *>(src);
        const float4 g = *reinterpret_cast<const float4 *>(src + HW);
        const float4 bl = *reinterpret_cast<const float4 *>(src + 2 * HW);
        const unsigned q[12] = {quantise(r.x), quantise(g.x), quantise(bl.x), quantise(r.y), quantise(g.y), quantise(bl.y),
                                quantise(r.z), quantise(g.z), quantise(bl.z), quantise(r.w), quantise(g.w), quantise(bl.w)};
        uint32_t *dst = reinterpret_cast<uint32_t *>(out + (size_t)i * 3);   // i % 4 == 0: 12 i is a multiple of 4
#pragma unroll
        for (int j = 0; j < 3; j++)
            dst[j] = q[4 * j] | (q[4 * j + 1] << 8) | (q[4 * j + 2] << 16) | (q[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) out[(size_t)i * 3 + c] = (uint8_t)quantise(src[(size_t)c * HW]);
    }
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_mapping_tile(void) { return MAP_T; }

extern "C" int g2s_mapping_fwd(const float *z, const float *w, const float *b, const float *center, float *out,
                               float *partial, int64_t N, int D, int L, int pixel_norm, float alpha, float gain,
                               float truncation, g2s_stream_t stream) {
    G2S_REQUIRE(z && w && b && out, "g2s_mapping_fwd: NULL pointer argument");
    G2S_REQUIRE(N >= 1, "g2s_mapping_fwd: N = %lld must be at least 1", (long long)N);
    G2S_REQUIRE(D >= 32 && D <= MAP_DMAX && D % 32 == 0,
                "g2s_mapping_fwd: D = %d (supported: multiples of 32 from 32 to %d)", D, MAP_DMAX);
    G2S_REQUIRE(L >= 1 && L <= 16, "g2s_mapping_fwd: L = %d outside 1..16", L);
    G2S_REQUIRE((((uintptr_t)z | (uintptr_t)w | (uintptr_t)out) & 15) == 0,
                "g2s_mapping_fwd: z, w and out must be 16-byte aligned");
    const long tiles = (N + MAP_T - 1) / MAP_T;
    G2S_REQUIRE(tiles <= 0x7fffffffL, "g2s_mapping_fwd: N = %lld exceeds the grid", (long long)N);
    MapParams p{};
    p.z = z;
    p.w = w;
    p.b = b;
    p.center = center;
    p.out = out;
    p.partial = partial;
    p.N = N;
    p.D = D;
    p.L = L;
    p.pixel_norm = pixel_norm ? 1 : 0;
    p.alpha = alpha;
    p.gain = gain;
    p.truncation = truncation;
    const int per_wave = (D / 16 + MAP_WAVES - 1) / MAP_WAVES;   // 16-column tiles per wave
    const dim3 grid((unsigned)tiles);
    hipStream_t st = as_stream(stream);
    if (per_wave <= 1) mapping_kernel<1><<<grid, 256, 0, st>>>(p);
    else if (per_wave <= 2) mapping_kernel<2><<<grid, 256, 0, st>>>(p);
    else if (per_wave <= 4) mapping_kernel<4><<<grid, 256, 0, st>>>(p);
    else mapping_kernel<8><<<grid, 256, 0, st>>>(p);
    return check_launch("g2s_mapping_fwd");
}

extern "C" int g2s_rows_mean(const float *partial, float *out, int64_t tiles, int D, int64_t N, g2s_stream_t stream) {
    G2S_REQUIRE(partial && out, "g2s_rows_mean: NULL pointer argument");
    G2S_REQUIRE(tiles >= 1 && D >= 1 && N >= 1, "g2s_rows_mean: sizes must be positive");
    rows_mean_kernel<<<cdiv(D, 256), 256, 0, as_stream(stream)>>>(partial, out, (long)tiles, D, (float)N);
    return check_launch("g2s_rows_mean");
}

extern "C" int g2s_image_to_u8(const float *x, uint8_t *out, int64_t B, int H, int W, g2s_stream_t stream) {
    G2S_REQUIRE(x && out, "g2s_image_to_u8: NULL pointer argument");
    G2S_REQUIRE(B >= 1 && H >= 1 && W >= 1, "g2s_image_to_u8: sizes must be positive");
    const long HW = (long)H * W;
    G2S_REQUIRE(B * HW <= 0x7fffffffL * 64, "g2s_image_to_u8: B * H * W exceeds the grid");
    const bool wide = HW % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0;
    if (wide) image_to_u8_kernel<4><<<cdiv(B * HW / 4, 256), 256, 0, as_stream(stream)>>>(x, out, B, HW);
    else image_to_u8_kernel<1><<<cdiv(B * HW, 256), 256, 0, as_stream(stream)>>>(x, out, B, HW);
    return check_launch("g2s_image_to_u8");
}
