// dataprep.hip — the data path of the vendored StyleGAN2 trainer (stylegan2-pytorch/prepare_data.py, dataset.py;
// here prepare_data.py and dataset.DeviceBatches).
//
// g2s_u8_batch   per iteration: gathers B samples of a packed planar uint8 dataset by index, mirrors the flagged
//                ones and converts to the float batch in [-1, 1] — one launch, indices and flags read on the device.
// g2s_resize_u8  once per dataset: Pillow's 8-bit resampler (ImagingResample: horizontal pass, intermediate rounded
//                to uint8, vertical pass; int32 accumulation of 22-bit fixed-point coefficients from 1 << 21) on the
//                centre-crop window only, interleaved in, planar out.  Integer arithmetic: exact.
//
// The passes of g2s_resize_u8 are two launches with a uint8 intermediate in global memory.  A fused launch would hold
// the horizontally resized rows of a tile in LDS; at 1024 -> 128 one output row needs 49 of them, so a workgroup
// either recomputes most of its horizontal rows for every few output rows or takes tens of KB of LDS and runs at one
// or two workgroups per CU.  The intermediate is 1 / scale of the input, written and read once, and the kernel runs
// once per dataset: the two launches cost less than that trade and keep each kernel a plain loop over its taps.
#include <algorithm>
#include <cstdint>
#include "g2s_common.h"

namespace g2s {

// t[v] = float(v) / 255 rounded to f32, then * 2 - 1 (dataset.ImageDataset: ToTensor's division, then the rescale).
// Evaluated by the compiler in IEEE f32: the division is correctly rounded, v / 255 * 2 is exact, so the subtraction
// is the second and last rounding — as in torch.
struct U8Table {
    float v[256];
    constexpr U8Table() : v() {
        for (int i = 0; i < 256; i++) v[i] = (float)i / 255.0f * 2.0f - 1.0f;
    }
};
__constant__ U8Table u8_table = U8Table();

__device__ __forceinline__ void load_table(float *t) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) t[i] = u8_table.v[i];
    __syncthreads();
}

// Wide path (S % 16 == 0; data, out 16-byte aligned): a lane owns 16 consecutive pixels of one row — one 16-byte
// load, four 16-byte stores.  A mirrored row reads the mirrored 16-byte chunk (aligned as well) and reverses it.
__global__ __launch_bounds__(256) void u8_batch_wide_kernel(const uint8_t *__restrict__ data, long N,
                                                            const int64_t *__restrict__ idx,
                                                            const uint8_t *__restrict__ flip, float *__restrict__ out,
                                                            long chunks, int per_sample, int per_row) {
    __shared__ float t[256];
    load_table(t);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (long)gridDim.x * blockDim.x) {
        const long b = i / per_sample;
        const int r = (int)(i - b * per_sample);        // chunk within the sample
        const int row = r / per_row, xc = r - row * per_row;
        const long n = idx[b];
        const bool f = flip[b] != 0;
        float4 *dst = reinterpret_cast<float4 *>(out) + i * 4;
        if (n < 0 || n >= N) {                           // never read outside the dataset: the batch shows NaN
            const float q = __builtin_nanf("");
            for (int j = 0; j < 4; j++) dst[j] = make_float4(q, q, q, q);
            continue;
        }
        const int sc = f ? per_row - 1 - xc : xc;
        const uint4 raw = reinterpret_cast<const uint4 *>(data)[(n * per_sample + (long)row * per_row) + sc];
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t d = f ? w[3 - j] : w[j];
            const float a = t[d & 255], bb = t[(d >> 8) & 255], c = t[(d >> 16) & 255], e = t[d >> 24];
            dst[j] = f ? make_float4(e, c, bb, a) : make_float4(a, bb, c, e);
        }
    }
}

// Scalar path: every other S and unaligned pointers.  A lane owns one output pixel.
__global__ __launch_bounds__(256) void u8_batch_scalar_kernel(const uint8_t *__restrict__ data, long N,
                                                              const int64_t *__restrict__ idx,
                                                              const uint8_t *__restrict__ flip,
                                                              float *__restrict__ out, long total, long per_sample,
                                                              int S) {
    __shared__ float t[256];
    load_table(t);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / per_sample;
        const long r = i - b * per_sample;
        const long row = r / S;
        const int x = (int)(r - row * S);
        const long n = idx[b];
        if (n < 0 || n >= N) {
            out[i] = __builtin_nanf("");
            continue;
        }
        out[i] = t[data[n * per_sample + row * S + (flip[b] ? S - 1 - x : x)]];
    }
}

__device__ __forceinline__ uint8_t clip8(int ss) { return (uint8_t)min(max(ss >> 22, 0), 255); }

// Horizontal pass (or the plain copy when kk is NULL): src [N, H, W, 3] interleaved -> dst [N, 3, rows, ow_c] planar,
// output rows row0 .. row0 + rows of the source, output columns left .. left + ow_c of the resized width.
// A lane owns one output pixel, all three channels.  The window is clamped to the row: a bad table cannot read
// outside src.
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                       const int32_t *__restrict__ kk,
                                                       const int32_t *__restrict__ bounds, int ks, long total, int H,
                                                       int W, int left, int ow_c, int row0, int rows) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % ow_c);
    const long q = i / ow_c;
    const int y = (int)(q % rows);
    const long n = q / rows;
    const uint8_t *line = src + ((n * H + row0 + y) * W) * 3;
    uint8_t r, g, b;
    if (kk) {
        const int xo = left + x;
        const int xmin = min(max(bounds[2 * xo], 0), W);
        const int cnt = min(min(bounds[2 * xo + 1], ks), W - xmin);
        const int32_t *k = kk + (long)xo * ks;
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int j = 0; j < cnt; j++) {
            const int c = k[j];
            const uint8_t *p = line + (xmin + j) * 3;
            s0 += p[0] * c;
            s1 += p[1] * c;
            s2 += p[2] * c;
        }
        r = clip8(s0), g = clip8(s1), b = clip8(s2);
    } else {
        const uint8_t *p = line + (left + x) * 3;
        r = p[0], g = p[1], b = p[2];
    }
    const long plane = (long)rows * ow_c;
    uint8_t *o = dst + n * 3 * plane + (long)y * ow_c + x;
    o[0] = r;
    o[plane] = g;
    o[2 * plane] = b;
}

// Vertical pass: in holds rows row0 .. row0 + rows of the (horizontally resized) image; element (n, c, y, x) is at
// n * sn + c * sc + (y - row0) * sy + x * sx, so it reads the planar intermediate or, when the horizontal pass is
// skipped, the interleaved source with x0 = left.  dst [N, 3, oh_c, ow_c] planar, output rows top .. top + oh_c.
// A lane owns one output value; the window is clamped to the rows that in holds.
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ dst,
                                                       const int32_t *__restrict__ kk,
                                                       const int32_t *__restrict__ bounds, int ks, long total, long sn,
                                                       long sc, long sy, long sx, int x0, int row0, int rows, int top,
                                                       int oh_c, int ow_c) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % ow_c);
    long q = i / ow_c;
    const int y = (int)(q % oh_c);
    q /= oh_c;
    const int c = (int)(q % 3);
    const long n = q / 3;
    const int yo = top + y;
    const int ymin = min(max(bounds[2 * yo], row0), row0 + rows);
    const int cnt = min(min(bounds[2 * yo + 1], ks), row0 + rows - ymin);
    const int32_t *k = kk + (long)yo * ks;
    const uint8_t *p = in + n * sn + c * sc + (long)(ymin - row0) * sy + (long)(x0 + x) * sx;
    int ss = 1 << 21;
    for (int j = 0; j < cnt; j++) ss += p[j * sy] * k[j];
    dst[i] = clip8(ss);
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_u8_batch(const uint8_t *data, int64_t N, const int64_t *idx, const uint8_t *flip, float *out, int B,
                            int S, g2s_stream_t stream) {
    G2S_REQUIRE(data && idx && flip && out, "NULL pointer argument");
    G2S_REQUIRE(N > 0 && B > 0 && S > 0, "N, B, S must be positive");
    G2S_REQUIRE(S <= 16384, "S too large");
    const long per_sample = 3L * S * S, total = per_sample * B;
    const bool aligned = ((reinterpret_cast<uintptr_t>(data) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (S % 16 == 0 && aligned) {
        const long chunks = total / 16;
        u8_batch_wide_kernel<<<(unsigned)std::min<long>((chunks + 255) / 256, 256 * 16), 256, 0, as_stream(stream)>>>(
            data, N, idx, flip, out, chunks, (int)(per_sample / 16), S / 16);
    } else {
        u8_batch_scalar_kernel<<<(unsigned)std::min<long>((total + 255) / 256, 256 * 16), 256, 0, as_stream(stream)>>>(
            data, N, idx, flip, out, total, per_sample, S);
    }
    return check_launch("g2s_u8_batch");
}

extern "C" int g2s_resize_u8(const uint8_t *src, uint8_t *dst, uint8_t *tmp, int N, int H, int W, int oh, int ow,
                             const int32_t *kx, const int32_t *bx, int ksx, const int32_t *ky, const int32_t *by,
                             int ksy, int left, int top, int ow_c, int oh_c, int row0, int rows, g2s_stream_t stream) {
    G2S_REQUIRE(src && dst, "NULL pointer argument");
    G2S_REQUIRE(N > 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && ow_c > 0 && oh_c > 0, "sizes must be positive");
    G2S_REQUIRE(left >= 0 && top >= 0 && left + (long)ow_c <= ow && top + (long)oh_c <= oh, "crop window outside the output");
    const bool horiz = ow != W, vert = oh != H;
    G2S_REQUIRE(!horiz || (kx && bx && ksx > 0), "ow != W needs the horizontal tables");
    G2S_REQUIRE(!vert || (ky && by && ksy > 0), "oh != H needs the vertical tables");
    if (!vert) row0 = top, rows = oh_c;     // the horizontal pass (or the copy) writes the window itself
    G2S_REQUIRE(row0 >= 0 && rows > 0 && row0 + (long)rows <= H, "intermediate rows outside the source");
    G2S_REQUIRE(!(horiz && vert) || tmp, "two passes need the intermediate buffer");
    G2S_REQUIRE((long)N * 3 * std::max<long>((long)H * W, (long)oh * ow) < (1L << 38), "tensor too large");
    hipStream_t st = as_stream(stream);
    if (horiz || !vert) {
        uint8_t *o = vert ? tmp : dst;
        const long total = (long)N * rows * ow_c;
        resize_h_kernel<<<cdiv(total, 256), 256, 0, st>>>(src, o, horiz ? kx : nullptr, bx, ksx, total, H, W, left, ow_c,
                                                           row0, rows);
        const int rc = check_launch("g2s_resize_u8 (horizontal)");
        if (rc != G2S_OK) return rc;
    }
    if (vert) {
        const long total = (long)N * 3 * oh_c * ow_c;
        if (horiz)
            resize_v_kernel<<<cdiv(total, 256), 256, 0, st>>>(tmp, dst, ky, by, ksy, total, 3L * rows * ow_c,
                                                               (long)rows * ow_c, ow_c, 1, 0, row0, rows, top, oh_c, ow_c);
        else
            resize_v_kernel<<<cdiv(total, 256), 256, 0, st>>>(src + (long)row0 * W * 3, dst, ky, by, ksy, total,
                                                               (long)H * W * 3, 1, 3L * W, 3, left, row0, rows, top, oh_c,
                                                               ow_c);
        return check_launch("g2s_resize_u8 (vertical)");
    }
    return G2S_OK;
}
