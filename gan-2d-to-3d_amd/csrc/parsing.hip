// parsing.hip — what the parsing networks behind the object masks (GAN2Shape/networks.py:247-586, resnet.py; used by
// MaskingModel, model.py:473-551) need beside g2s_conv2d.  All fp32, no float atomics: every result is
// bit-reproducible from run to run.
//
//   g2s_conv_stem7        7x7 stride-2 pad-3 convolution from 3 channels, bias + ReLU      (ResNet-18 stem; k > 5)
//   g2s_maxpool3x3s2      3x3 stride-2 pad-1 max pool, padding = -inf
//   g2s_adaptive_avgpool  PyTorch's adaptive average pool (global pools, PPM bins, area down-sampling)
//   g2s_resize_bilinear   bilinear resize, align_corners on or off
//   g2s_gate_add_act      y = act(x * s'[b,c] + t[b,c] + r[b,c,h,w])   (residual add, attention gates)
//   g2s_parse_head        low-resolution logits -> area-averaged object mask / confidence map; the full-resolution
//                         logits exist only in registers
#include <algorithm>
#include <cstdint>
#include "g2s_common.h"
#include "wave_sum.h"

namespace g2s {

// ------------------------------------------------------------------ 7x7 stem
// A workgroup computes a 16 x 16 tile of output pixels for STEM_MC output channels: the 37 x 37 x 3 input patch
// sits in LDS, a thread owns one pixel and STEM_MC accumulators, and the weight index is uniform over the
// workgroup (read through the scalar cache).  grid (tiles, ceil(M / STEM_MC), B)
constexpr int STEM_T = 16, STEM_P = 2 * STEM_T + 5, STEM_MC = 16;

__global__ __launch_bounds__(256) void conv_stem7_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         const float *__restrict__ bias, float *__restrict__ y,
                                                         int M, int H, int W, int OH, int OW, int tiles_x, int relu) {
    __shared__ float patch[3][STEM_P][STEM_P];
    const int b = blockIdx.z, m0 = blockIdx.y * STEM_MC;
    const int ty0 = (blockIdx.x / tiles_x) * STEM_T, tx0 = (blockIdx.x % tiles_x) * STEM_T;
    const int iy0 = 2 * ty0 - 3, ix0 = 2 * tx0 - 3;
    const float *xb = x + (size_t)b * 3 * H * W;
    for (int i = threadIdx.x; i < 3 * STEM_P * STEM_P; i += 256) {
        const int c = i / (STEM_P * STEM_P), rem = i - c * STEM_P * STEM_P;
        const int py = rem / STEM_P, px = rem - py * STEM_P;
        const int iy = iy0 + py, ix = ix0 + px;
        patch[c][py][px] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xb[((size_t)c * H + iy) * W + ix] : 0.0f;
    }
    __syncthreads();
    const int ty = threadIdx.x / STEM_T, tx = threadIdx.x % STEM_T;
    float acc[STEM_MC];
#pragma unroll
    for (int m = 0; m < STEM_MC; ++m) acc[m] = 0.0f;
    for (int c = 0; c < 3; ++c)
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float v = patch[c][2 * ty + ky][2 * tx + kx];
                const int tap = c * 49 + ky * 7 + kx;
#pragma unroll
                for (int m = 0; m < STEM_MC; ++m) {
                    const int mm = min(m0 + m, M - 1);          // past M: a valid address, the result is dropped
                    acc[m] = fmaf(v, w[(size_t)mm * 147 + tap], acc[m]);
                }
            }
    const int oy = ty0 + ty, ox = tx0 + tx;
    if (oy >= OH || ox >= OW) return;
#pragma unroll
    for (int m = 0; m < STEM_MC; ++m) {
        if (m0 + m >= M) break;
        float v = acc[m] + (bias ? bias[m0 + m] : 0.0f);
        if (relu) v = fmaxf(v, 0.0f);
        y[(((size_t)b * M + m0 + m) * OH + oy) * OW + ox] = v;
    }
}

// ------------------------------------------------------------------ pools, resize, gate
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                           long n, int H, int W, int OH, int OW) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const long p = i / ((long)OW * OH);
    const float *in = x + p * H * W;
    float v = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix >= 0 && ix < W) v = fmaxf(v, in[(long)iy * W + ix]);
        }
    }
    y[i] = v;
}

// One wave per output: its lanes stride over the bin, then a butterfly sum (one fixed order).
__global__ __launch_bounds__(256) void adaptive_avgpool_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                               long n, int H, int W, int OH, int OW) {
    const long o = (long)blockIdx.x * 4 + threadIdx.x / 64;
    if (o >= n) return;
    const int lane = threadIdx.x & 63;
    const int ox = (int)(o % OW), oy = (int)((o / OW) % OH);
    const long p = o / ((long)OW * OH);
    const int h0 = (int)((long)oy * H / OH), h1 = (int)(((long)(oy + 1) * H + OH - 1) / OH);
    const int w0 = (int)((long)ox * W / OW), w1 = (int)(((long)(ox + 1) * W + OW - 1) / OW);
    const int bw = w1 - w0, cnt = (h1 - h0) * bw;
    const float *in = x + p * H * W;
    float acc = 0.0f;
    for (int i = lane; i < cnt; i += 64) {
        const int r = i / bw;
        acc += in[(long)(h0 + r) * W + w0 + (i - r * bw)];
    }
    acc = wave_sum(acc);
    if (lane == 0) y[o] = acc / (float)cnt;
}

// Source index and weight of one output coordinate, as ATen computes them in fp32.
__device__ __forceinline__ void bilinear_tap(int dst, float scale, int align, int in, int &i0, int &i1, float &l1) {
    float src = align ? scale * (float)dst : scale * ((float)dst + 0.5f) - 0.5f;
    src = fmaxf(src, 0.0f);
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                              long n, int H, int W, int OH, int OW, float sh,
                                                              float sw, int align) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const long p = i / ((long)OW * OH);
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_tap(oy, sh, align, H, y0, y1, ly);
    bilinear_tap(ox, sw, align, W, x0, x1, lx);
    const float *in = x + p * H * W;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    y[i] = hy * (hx * in[(long)y0 * W + x0] + lx * in[(long)y0 * W + x1]) +
           ly * (hx * in[(long)y1 * W + x0] + lx * in[(long)y1 * W + x1]);
}

__device__ __forceinline__ float gate_of(float s, int sigmoid, int plus_one) {
    if (sigmoid) s = 1.0f / (1.0f + expf(-s));
    return plus_one ? s + 1.0f : s;
}

// V = 4: float4 accesses (HW % 4 == 0 and 16-byte aligned pointers, checked by the launcher), else V = 1.
template <int V>
__global__ __launch_bounds__(256) void gate_add_act_kernel(const float *__restrict__ x, const float *__restrict__ s,
                                                           const float *__restrict__ t, const float *__restrict__ r,
                                                           float *__restrict__ y, long n, int HW, int sigmoid,
                                                           int plus_one, int relu) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n) return;
    const long bc = i / HW;
    const float g = s ? gate_of(s[bc], sigmoid, plus_one) : 1.0f;
    const float off = t ? t[bc] : 0.0f;
    float xv[V], rv[V];
    if (V == 4) {
        *reinterpret_cast<float4 *>(xv) = *reinterpret_cast<const float4 *>(x + i);
        if (r) *reinterpret_cast<float4 *>(rv) = *reinterpret_cast<const float4 *>(r + i);
    } else {
        xv[0] = x[i];
        if (r) rv[0] = r[i];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float v = s ? xv[j] * g : xv[j];
        if (t) v += off;
        if (r) v += rv[j];
        xv[j] = relu ? fmaxf(v, 0.0f) : v;
    }
    if (V == 4) *reinterpret_cast<float4 *>(y + i) = *reinterpret_cast<float4 *>(xv);
    else y[i] = xv[0];
}

// ------------------------------------------------------------------ parse head
__device__ __forceinline__ unsigned enc_ordered(float f) {      // a < b  <=>  enc(a) < enc(b)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_ordered(unsigned e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

struct ParseArgs {
    int C, h, w, size, S, mode, drop;
    unsigned set;
    float sh, sw;
};

// Workspace words of sample b: ws[4 b] = max of ~enc(v) (the min), ws[4 b + 1] = max of enc(v), ws[4 b + 2] = number
// of full-resolution pixels of the class; cleared by the launcher.
// One wave per output pixel: its lanes stride over the pixels of the area bin, each interpolates the C logits at
// its pixel and applies the rule; butterfly sums give the bin's average.  Bins overlap when size / S is not an
// integer; a pixel is counted (and its full-resolution mask byte written) by the one bin that owns it, the bin
// whose first row / column is the last one at or before the pixel.  grid (ceil(S*S / 4), B)
__global__ __launch_bounds__(256) void parse_head_kernel(const float *__restrict__ logits, float *__restrict__ out,
                                                         uint8_t *__restrict__ full, unsigned *__restrict__ ws,
                                                         ParseArgs a) {
    __shared__ unsigned red[3][4];
    const int b = blockIdx.y, wave = threadIdx.x / 64, lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + wave;
    const int S = a.S, size = a.size;
    float acc = 0.0f, vmin = INFINITY, vmax = -INFINITY;
    unsigned owned_pos = 0;
    if (o < S * S) {
        const int oy = o / S, ox = o - oy * S;
        const int y0 = (int)((long)oy * size / S), y1 = (int)(((long)(oy + 1) * size + S - 1) / S);
        const int x0 = (int)((long)ox * size / S), x1 = (int)(((long)(ox + 1) * size + S - 1) / S);
        const int yown = (int)((long)(oy + 1) * size / S), xown = (int)((long)(ox + 1) * size / S);
        const int bw = x1 - x0, cnt = (y1 - y0) * bw;
        const float *lb = logits + (size_t)b * a.C * a.h * a.w;
        const int plane = a.h * a.w;
        for (int i = lane; i < cnt; i += 64) {
            const int ry = i / bw, py = y0 + ry, px = x0 + (i - ry * bw);
            int iy0, iy1, ix0, ix1;
            float ly, lx;
            bilinear_tap(py, a.sh, 1, a.h, iy0, iy1, ly);
            bilinear_tap(px, a.sw, 1, a.w, ix0, ix1, lx);
            const float hy = 1.0f - ly, hx = 1.0f - lx;
            const int o00 = iy0 * a.w + ix0, o01 = iy0 * a.w + ix1, o10 = iy1 * a.w + ix0, o11 = iy1 * a.w + ix1;
            float value;
            if (a.mode == 0) {
                float best = -INFINITY;
                int cls = -1;
                for (int c = 0; c < a.C; ++c) {
                    if (c == a.drop) continue;
                    const float *p = lb + (size_t)c * plane;
                    const float v = hy * (hx * p[o00] + lx * p[o01]) + ly * (hx * p[o10] + lx * p[o11]);
                    if (cls < 0 || v > best) { best = v; cls = c; }
                }
                const unsigned member = (a.set >> cls) & 1u;
                value = (float)member;
                if (py < yown && px < xown) {
                    owned_pos += member;
                    if (full) full[((size_t)b * size + py) * size + px] = (uint8_t)member;
                }
            } else {
                value = 0.0f;
                for (int c = 0; c < a.C; ++c) {
                    if (!((a.set >> c) & 1u)) continue;
                    const float *p = lb + (size_t)c * plane;
                    value += hy * (hx * p[o00] + lx * p[o01]) + ly * (hx * p[o10] + lx * p[o11]);
                }
                vmin = fminf(vmin, value);
                vmax = fmaxf(vmax, value);
            }
            acc += value;
        }
        acc = wave_sum(acc);
        if (lane == 0) out[(size_t)b * S * S + o] = acc / (float)cnt;
    }
    // per-workgroup partials, then at most one atomic per word and workgroup (integer max / add: exact, order-free)
    unsigned nmin = ~enc_ordered(vmin), emax = enc_ordered(vmax);
    for (int off = 32; off > 0; off >>= 1) {
        nmin = max(nmin, (unsigned)__shfl_xor((int)nmin, off));
        emax = max(emax, (unsigned)__shfl_xor((int)emax, off));
        owned_pos += (unsigned)__shfl_xor((int)owned_pos, off);
    }
    if (lane == 0) { red[0][wave] = nmin; red[1][wave] = emax; red[2][wave] = owned_pos; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned *slot = ws + 4 * b;
        if (a.mode == 0) {
            const unsigned pos = red[2][0] + red[2][1] + red[2][2] + red[2][3];
            if (pos) atomicAdd(slot + 2, pos);
        } else {
            nmin = max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3]));
            emax = max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3]));
            // the words only grow: a stale read can only let a needless atomic through
            if (nmin > __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMax(slot, nmin);
            if (emax > __atomic_load_n(slot + 1, __ATOMIC_RELAXED)) atomicMax(slot + 1, emax);
        }
    }
}

// Normalisation (confidence) or the all-ones fallback (hard mask).  grid (ceil(max(S*S, size*size if full) / 256), B)
__global__ __launch_bounds__(256) void parse_finish_kernel(float *__restrict__ out, uint8_t *__restrict__ full,
                                                           int *__restrict__ fallback,
                                                           const unsigned *__restrict__ ws, int S, int size,
                                                           int mode) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned *slot = ws + 4 * b;
    if (mode == 0) {
        const bool empty = slot[2] == 0u;
        if (i == 0 && fallback) fallback[b] = empty ? 1 : 0;
        if (!empty) return;
        if (i < S * S) out[(size_t)b * S * S + i] = 1.0f;
        if (full && i < size * size) full[(size_t)b * size * size + i] = 1;
    } else {
        if (i == 0 && fallback) fallback[b] = 0;
        if (i >= S * S) return;
        const float lo = dec_ordered(~slot[0]), hi = dec_ordered(slot[1]);
        const size_t k = (size_t)b * S * S + i;
        out[k] = (out[k] - lo) / (hi - lo);
    }
}

static bool fits_int(long v) { return v > 0 && v < (1l << 31); }

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_conv_stem7(const float *x, const float *w, const float *bias, float *y, int B, int M, int H, int W,
                              int relu, g2s_stream_t stream) {
    G2S_REQUIRE(B >= 0 && M > 0 && H > 0 && W > 0, "g2s_conv_stem7: sizes must be positive");
    if (B == 0) return G2S_OK;
    G2S_REQUIRE(x && w && y, "g2s_conv_stem7: x, w, y must not be NULL");
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    G2S_REQUIRE(B <= 65535 && cdiv(M, STEM_MC) <= 65535 && fits_int((long)B * 3 * H * W) &&
                    fits_int((long)B * M * OH * OW),
                "g2s_conv_stem7: problem too large");
    const int tiles_x = cdiv(OW, STEM_T), tiles_y = cdiv(OH, STEM_T);
    conv_stem7_kernel<<<dim3(tiles_x * tiles_y, cdiv(M, STEM_MC), B), 256, 0, as_stream(stream)>>>(
        x, w, bias, y, M, H, W, OH, OW, tiles_x, relu != 0);
    return check_launch("g2s_conv_stem7");
}

extern "C" int g2s_maxpool3x3s2(const float *x, float *y, int planes, int H, int W, g2s_stream_t stream) {
    G2S_REQUIRE(planes >= 0 && H > 0 && W > 0, "g2s_maxpool3x3s2: sizes must be positive");
    if (planes == 0) return G2S_OK;
    G2S_REQUIRE(x && y, "g2s_maxpool3x3s2: x, y must not be NULL");
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    G2S_REQUIRE(fits_int((long)planes * H * W), "g2s_maxpool3x3s2: problem too large");
    const long n = (long)planes * OH * OW;
    maxpool3x3s2_kernel<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(x, y, n, H, W, OH, OW);
    return check_launch("g2s_maxpool3x3s2");
}

extern "C" int g2s_adaptive_avgpool(const float *x, float *y, int planes, int H, int W, int out_h, int out_w,
                                    g2s_stream_t stream) {
    G2S_REQUIRE(planes >= 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, "g2s_adaptive_avgpool: sizes must be positive");
    if (planes == 0) return G2S_OK;
    G2S_REQUIRE(x && y, "g2s_adaptive_avgpool: x, y must not be NULL");
    G2S_REQUIRE(fits_int((long)planes * H * W) && fits_int((long)planes * out_h * out_w),
                "g2s_adaptive_avgpool: problem too large");
    const long n = (long)planes * out_h * out_w;
    adaptive_avgpool_kernel<<<cdiv(n, 4), 256, 0, as_stream(stream)>>>(x, y, n, H, W, out_h, out_w);
    return check_launch("g2s_adaptive_avgpool");
}

extern "C" int g2s_resize_bilinear(const float *x, float *y, int planes, int H, int W, int out_h, int out_w,
                                   int align_corners, g2s_stream_t stream) {
    G2S_REQUIRE(planes >= 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, "g2s_resize_bilinear: sizes must be positive");
    if (planes == 0) return G2S_OK;
    G2S_REQUIRE(x && y, "g2s_resize_bilinear: x, y must not be NULL");
    G2S_REQUIRE(fits_int((long)planes * H * W) && fits_int((long)planes * out_h * out_w),
                "g2s_resize_bilinear: problem too large");
    const int al = align_corners != 0;
    const float sh = al ? (out_h > 1 ? (float)(H - 1) / (float)(out_h - 1) : 0.0f) : (float)H / (float)out_h;
    const float sw = al ? (out_w > 1 ? (float)(W - 1) / (float)(out_w - 1) : 0.0f) : (float)W / (float)out_w;
    const long n = (long)planes * out_h * out_w;
    resize_bilinear_kernel<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(x, y, n, H, W, out_h, out_w, sh, sw, al);
    return check_launch("g2s_resize_bilinear");
}

extern "C" int g2s_gate_add_act(const float *x, const float *s, const float *t, const float *r, float *y, int planes,
                                int HW, int sigmoid, int plus_one, int relu, g2s_stream_t stream) {
    G2S_REQUIRE(planes >= 0 && HW > 0, "g2s_gate_add_act: sizes must be positive");
    if (planes == 0) return G2S_OK;
    G2S_REQUIRE(x && y, "g2s_gate_add_act: x, y must not be NULL");
    G2S_REQUIRE(s || !(sigmoid || plus_one), "g2s_gate_add_act: sigmoid / plus_one need the gate s");
    G2S_REQUIRE(fits_int((long)planes * HW), "g2s_gate_add_act: problem too large");
    const long n = (long)planes * HW;
    const uintptr_t bits = (uintptr_t)x | (uintptr_t)y | (uintptr_t)r;
    if (HW % 4 == 0 && bits % 16 == 0)
        gate_add_act_kernel<4><<<cdiv(n / 4, 256), 256, 0, as_stream(stream)>>>(x, s, t, r, y, n, HW, sigmoid != 0,
                                                                                plus_one != 0, relu != 0);
    else
        gate_add_act_kernel<1><<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(x, s, t, r, y, n, HW, sigmoid != 0,
                                                                            plus_one != 0, relu != 0);
    return check_launch("g2s_gate_add_act");
}

extern "C" size_t g2s_parse_head_workspace_bytes(int B) { return B > 0 ? (size_t)B * 16 : 0; }

extern "C" int g2s_parse_head(const float *logits, int B, int C, int h, int w, int size, int S, int mode, int drop,
                              uint32_t class_set, float *out, uint8_t *full_mask, int *fallback, void *workspace,
                              size_t workspace_bytes, g2s_stream_t stream) {
    G2S_REQUIRE(B >= 0 && B <= 65535, "g2s_parse_head: B must be in 0..65535");
    G2S_REQUIRE(C >= 1 && C <= 32, "g2s_parse_head: C must be in 1..32 (got %d)", C);
    G2S_REQUIRE(h > 0 && w > 0 && size > 0 && size <= 16384, "g2s_parse_head: h, w, size must be positive, size <= 16384");
    G2S_REQUIRE(S >= 1 && S <= size, "g2s_parse_head: S must be in 1..size (area average down)");
    G2S_REQUIRE(mode == 0 || mode == 1, "g2s_parse_head: mode must be 0 (hard mask) or 1 (confidence)");
    G2S_REQUIRE(drop >= -1 && drop < C, "g2s_parse_head: drop must be -1 or a channel");
    G2S_REQUIRE(!(mode == 0 && drop >= 0 && C == 1), "g2s_parse_head: no channel left after the drop");
    G2S_REQUIRE(!(mode == 1 && drop != -1), "g2s_parse_head: the confidence sum takes no dropped channel");
    G2S_REQUIRE(class_set != 0 && (C == 32 || (class_set >> C) == 0), "g2s_parse_head: class_set must name channels below C");
    G2S_REQUIRE(!(mode == 1 && full_mask), "g2s_parse_head: the full-resolution mask belongs to the hard mode");
    if (B == 0) return G2S_OK;
    G2S_REQUIRE(logits && out, "g2s_parse_head: logits, out must not be NULL");
    G2S_REQUIRE(fits_int((long)B * C * h * w) && fits_int((long)B * size * size), "g2s_parse_head: problem too large");
    const size_t need = g2s_parse_head_workspace_bytes(B);
    if (!workspace || workspace_bytes < need)
        return fail(G2S_ERR_WORKSPACE, "g2s_parse_head: workspace of %zu bytes, %zu needed",
                    workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess)
        return fail(G2S_ERR_LAUNCH, "g2s_parse_head: hipMemsetAsync failed");
    ParseArgs a{C, h, w, size, S, mode, drop, class_set,
                size > 1 ? (float)(h - 1) / (float)(size - 1) : 0.0f,
                size > 1 ? (float)(w - 1) / (float)(size - 1) : 0.0f};
    unsigned *ws = static_cast<unsigned *>(workspace);
    parse_head_kernel<<<dim3(cdiv((long)S * S, 4), B), 256, 0, st>>>(logits, out, full_mask, ws, a);
    int rc = check_launch("g2s_parse_head");
    if (rc != G2S_OK) return rc;
    const long cover = std::max((long)S * S, full_mask ? (long)size * size : 0l);
    parse_finish_kernel<<<dim3(cdiv(cover, 256), B), 256, 0, st>>>(out, full_mask, fallback, ws, S, size, mode);
    return check_launch("g2s_parse_head (finish)");
}
