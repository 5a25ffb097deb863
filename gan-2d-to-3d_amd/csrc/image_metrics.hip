// image_metrics.hip — how well one image reproduces another, per image of a batch: count, MAE, MSE, PSNR over the
// masked pixels and the mean structural similarity (SSIM, Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, windows
// wholly inside the image) over the masked window centres.  include/g2s.h (g2s_image_metrics) states the definitions.
// The torch composition (ten 1-D convolutions, about twenty pointwise and reduction launches) becomes two launches.
//
//   image_metrics_tiles   grid (tiles_x, tiles_y, B), 256 threads: one IM_TX x IM_TY tile of window centres of one
//                         image per workgroup.  The mask of the tile and its 5-pixel halo is thresholded into LDS once;
//                         then, channel by channel, the tile + halo of a and b is staged in LDS (every value is read
//                         from memory once per workgroup), a horizontal pass writes the five moments (a, b, a^2, b^2,
//                         ab) filtered along x to LDS, and a vertical pass filters them along y and evaluates SSIM in
//                         registers, two centres per thread.  The pixel sums (count, |d|, d^2) are taken while staging,
//                         over the pixels the tile OWNS: its centre region, extended to the image border by the first
//                         and last tile of each axis — the 5-pixel frame that no window centre covers is counted once,
//                         the halo (owned by the neighbours) never.  An image narrower or lower than a window has one
//                         tile per such axis, which owns all of it and has no centre.
//                         The five terms are summed in double over the wave (xor butterfly), then over the four waves
//                         in wave order, and written to partials[b][tile][5].
//   image_metrics_finish  grid B, one wave: lane l adds tiles l, l + 64, ... in that order, a butterfly joins the
//                         lanes, lane 0 writes out[b][6].
//
// Every sum has one fixed order whatever the launch: no atomics, bit-identical from run to run and in either mode of
// g2s_set_deterministic.  The filter runs in double: products of two floats are exact there, so E[a^2] - E[a]^2 loses
// nothing to the sum, and a 33 KB moment buffer is what it costs.  The file is compiled with -ffp-contract=off: for
// a == b numerator and denominator of SSIM are then the same bits and the map is exactly 1.
#include <cmath>
#include "g2s_common.h"
#include "wave_sum.h"

namespace g2s {

constexpr int IM_TX = 32, IM_TY = 16;          // tile of window centres
constexpr int IM_R = 5, IM_WIN = 2 * IM_R + 1; // window radius and size
constexpr int IM_LX = IM_TX + 2 * IM_R, IM_LY = IM_TY + 2 * IM_R;
constexpr int IM_MOMENTS = 5;                  // a, b, a^2, b^2, ab
constexpr int IM_TERMS = 5;                    // n, sum |d|, sum d^2, n_windows, sum ssim
constexpr double IM_SIGMA = 1.5, IM_K1 = 0.01, IM_K2 = 0.03;

struct ImWindow {
    double w[IM_WIN];
};

__global__ __launch_bounds__(256) void image_metrics_tiles(const float *__restrict__ a, const float *__restrict__ b,
                                                           const float *__restrict__ mask, int C, int H, int W, double c1,
                                                           double c2, ImWindow win, double *__restrict__ partials) {
    __shared__ float sa[IM_LY][IM_LX], sb[IM_LY][IM_LX];
    __shared__ unsigned char sm[IM_LY][IM_LX];
    __shared__ double sh[IM_MOMENTS][IM_LY][IM_TX];
    __shared__ double red[4][IM_TERMS];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * IM_TX, oy = blockIdx.y * IM_TY;      // image position of the staged region's corner
    // the pixels this tile owns for the pixel sums
    const int own_x0 = blockIdx.x == 0 ? 0 : ox + IM_R, own_x1 = blockIdx.x == gridDim.x - 1 ? W : ox + IM_R + IM_TX;
    const int own_y0 = blockIdx.y == 0 ? 0 : oy + IM_R, own_y1 = blockIdx.y == gridDim.y - 1 ? H : oy + IM_R + IM_TY;
    const size_t plane = (size_t)H * W;

    for (int i = tid; i < IM_LY * IM_LX; i += 256) {
        const int ly = i / IM_LX, lx = i - ly * IM_LX;
        const int y = oy + ly, x = ox + lx;
        bool m = y < H && x < W;
        if (m && mask) m = mask[(size_t)blockIdx.z * plane + (size_t)y * W + x] > 0.5f;
        sm[ly][lx] = m ? 1 : 0;
    }
    // no barrier: the staging loop below reads sm[i] in the thread that wrote it; the centres read it after barriers

    double term[IM_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; c++) {
        const size_t image = ((size_t)blockIdx.z * C + c) * plane;
        for (int i = tid; i < IM_LY * IM_LX; i += 256) {
            const int ly = i / IM_LX, lx = i - ly * IM_LX;
            const int y = oy + ly, x = ox + lx;
            float pa = 0.0f, pb = 0.0f;
            if (y < H && x < W) {
                const size_t at = image + (size_t)y * W + x;
                pa = a[at];
                pb = b[at];
                if (sm[ly][lx] && x >= own_x0 && x < own_x1 && y >= own_y0 && y < own_y1) {
                    const double d = (double)pa - (double)pb;
                    if (c == 0) term[0] += 1.0;
                    term[1] += fabs(d);
                    term[2] += d * d;
                }
            }
            sa[ly][lx] = pa;
            sb[ly][lx] = pb;
        }
        __syncthreads();      // also: the previous channel's vertical pass has left sh

        // horizontal pass: row r of the staged region, centre column cx -> the five moments filtered along x
        for (int i = tid; i < IM_LY * IM_TX; i += 256) {
            const int r = i / IM_TX, cx = i - r * IM_TX;
            if (oy + r >= H || ox + cx + 2 * IM_R >= W) continue;      // no window reads this entry
            double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
            for (int j = 0; j < IM_WIN; j++) {
                const double va = (double)sa[r][cx + j], vb = (double)sb[r][cx + j], w = win.w[j];
                m0 += w * va;
                m1 += w * vb;
                m2 += w * (va * va);
                m3 += w * (vb * vb);
                m4 += w * (va * vb);
            }
            sh[0][r][cx] = m0;
            sh[1][r][cx] = m1;
            sh[2][r][cx] = m2;
            sh[3][r][cx] = m3;
            sh[4][r][cx] = m4;
        }
        __syncthreads();      // also: sa / sb are free for the next channel

        // vertical pass and SSIM: thread (cx, cy) has the centres of tile rows cy and cy + 8
        const int cx = tid & (IM_TX - 1);
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int cy = (tid >> 5) + half * (IM_TY / 2);
            if (ox + cx + 2 * IM_R >= W || oy + cy + 2 * IM_R >= H || !sm[cy + IM_R][cx + IM_R]) continue;
            double mom[IM_MOMENTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < IM_WIN; j++)
#pragma unroll
                for (int k = 0; k < IM_MOMENTS; k++) mom[k] += win.w[j] * sh[k][cy + j][cx];
            const double mu_a = mom[0], mu_b = mom[1];
            const double var_a = mom[2] - mu_a * mu_a, var_b = mom[3] - mu_b * mu_b, cov = mom[4] - mu_a * mu_b;
            const double num = (2.0 * mu_a * mu_b + c1) * (2.0 * cov + c2);
            const double den = (mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2);
            if (c == 0) term[3] += 1.0;
            term[4] += num / den;
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < IM_TERMS; k++) {
        const double v = wave_sum(term[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < IM_TERMS) {
        const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partials[tile * IM_TERMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

__global__ __launch_bounds__(64) void image_metrics_finish(const double *__restrict__ partials, int tiles, int C,
                                                          double range2, float *__restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double *p = partials + (size_t)b * tiles * IM_TERMS;
    double acc[IM_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = lane; t < tiles; t += 64)
#pragma unroll
        for (int k = 0; k < IM_TERMS; k++) acc[k] += p[(size_t)t * IM_TERMS + k];
#pragma unroll
    for (int k = 0; k < IM_TERMS; k++) acc[k] = wave_sum(acc[k]);
    if (lane != 0) return;
    float *o = out + (size_t)b * 6;
    const float nan = __builtin_nanf("");
    const double n = acc[0], nw = acc[3];
    o[0] = (float)n;
    if (n == 0.0) {
        o[1] = o[2] = o[3] = nan;
    } else {
        const double mse = acc[2] / (n * C);
        o[1] = (float)(acc[1] / (n * C));
        o[2] = (float)mse;
        o[3] = mse == 0.0 ? __builtin_inff() : (float)(10.0 * log10(range2 / mse));
    }
    o[4] = (float)nw;
    o[5] = nw == 0.0 ? nan : (float)(acc[4] / (nw * C));
}

// tiles of window centres along an axis of n pixels; an axis shorter than a window still has one (without a centre)
static int im_axis_tiles(int n, int tile) { return n > 2 * IM_R ? cdiv(n - 2 * IM_R, tile) : 1; }
static size_t im_tiles(int H, int W) { return (size_t)im_axis_tiles(W, IM_TX) * im_axis_tiles(H, IM_TY); }

}  // namespace g2s

using namespace g2s;

extern "C" size_t g2s_image_metrics_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * im_tiles(H, W) * IM_TERMS * sizeof(double);
}

extern "C" int g2s_image_metrics(const float *a, const float *b, const float *mask, int B, int C, int H, int W,
                                 float data_range, float *out, void *workspace, size_t workspace_bytes,
                                 g2s_stream_t stream) {
    G2S_REQUIRE(a && b && out, "g2s_image_metrics: NULL pointer");
    G2S_REQUIRE(B > 0 && B <= 65535, "g2s_image_metrics: B = %d outside [1, 65535]", B);
    G2S_REQUIRE(C >= 1 && C <= 4, "g2s_image_metrics: C = %d outside [1, 4]", C);
    G2S_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "g2s_image_metrics: H = %d, W = %d outside [1, 32768]", H, W);
    G2S_REQUIRE(data_range > 0.0f && std::isfinite(data_range), "g2s_image_metrics: data_range = %g must be positive and finite",
                (double)data_range);
    const size_t need = g2s_image_metrics_workspace_bytes(B, C, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(G2S_ERR_WORKSPACE, "g2s_image_metrics: workspace of %zu bytes, %zu needed",
                    workspace ? workspace_bytes : (size_t)0, need);
    G2S_REQUIRE(((uintptr_t)workspace & 7) == 0, "g2s_image_metrics: workspace must be 8-byte aligned");
    ImWindow win;
    double sum = 0.0;
    for (int j = 0; j < IM_WIN; j++) {
        const double x = (double)(j - IM_R);
        win.w[j] = exp(-(x * x) / (2.0 * IM_SIGMA * IM_SIGMA));
        sum += win.w[j];
    }
    for (int j = 0; j < IM_WIN; j++) win.w[j] /= sum;
    const double L = (double)data_range;
    const double c1 = (IM_K1 * L) * (IM_K1 * L), c2 = (IM_K2 * L) * (IM_K2 * L);
    hipStream_t st = as_stream(stream);
    double *partials = (double *)workspace;
    image_metrics_tiles<<<dim3(im_axis_tiles(W, IM_TX), im_axis_tiles(H, IM_TY), B), 256, 0, st>>>(a, b, mask, C, H, W, c1, c2,
                                                                                                 win, partials);
    image_metrics_finish<<<B, 64, 0, st>>>(partials, (int)im_tiles(H, W), C, L * L, out);
    return check_launch("g2s_image_metrics");
}
