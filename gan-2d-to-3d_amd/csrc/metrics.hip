// metrics.hip — depth and normal accuracy of a recovered depth map against a ground-truth one, per image:
// count, masked MAE and MSE, scale-invariant depth error (SIDE) and mean angle deviation of the normals
// (MAD, degrees): the figures of the BFM table of the GAN2Shape / Unsup3D papers.  The torch composition
// (two 3x3 avg_pool2d + threshold, two logs, a two-pass second moment, two get_normal_from_depth chains, the
// angle, five masked sums) is about 40 launches; this is two.
//
//   depth_metrics_tiles   grid (ceil(W/32), ceil(H/8), B), 256 threads: one 32 x 8 tile per workgroup.  The tile
//                         and its one-pixel halo (both depths, a validity byte) are staged in LDS, 34 x 10 x 9
//                         bytes: every depth and mask value is loaded from memory once per workgroup, the
//                         halo's second reader hits L2.  Each thread owns one pixel: 3x3 erosion and the
//                         normals' stencil come from LDS.  The seven per-pixel terms are summed in double over
//                         the wave (xor butterfly), then over the four waves in wave order, and written
//                         to partials[b][tile][7].
//   depth_metrics_finish  grid B, one wave: lane l adds tiles l, l + 64, ... in that order, a butterfly joins the
//                         lanes, lane 0 writes out[b][5].
//
// Every sum has one fixed order whatever the launch: no atomics, no ticket, bit-identical from run to run.
// SIDE: the moments of delta = log p - log g are held in double (log in double as well), so that
// E[delta^2] - E[delta]^2 keeps 1e-16 of E[delta^2] and p = c g gives rounding noise of the inputs, not of the sum.
// The file is compiled with -ffp-contract=off: d2 / n - mean * mean is then exactly 0 for a single pixel.
#include "g2s_common.h"
#include "wave_sum.h"
#include "normal_core.h"

namespace g2s {

constexpr int MT_X = 32, MT_Y = 8;            // tile
constexpr int MT_LX = MT_X + 2, MT_LY = MT_Y + 2;
constexpr int MT_TERMS = 7;                   // n, sum |d|, sum d^2, sum delta, sum delta^2, n_mad, sum angle
constexpr unsigned char PIX_VALID = 1, PIX_FINITE = 2;

__global__ __launch_bounds__(256) void depth_metrics_tiles(const float *__restrict__ pred, const float *__restrict__ gt,
                                                           const float *__restrict__ mask_pred,
                                                           const float *__restrict__ mask_gt,
                                                           const float *__restrict__ rays, int H, int W, int erode,
                                                           double *__restrict__ partials) {
    __shared__ float sp[MT_LY][MT_LX], sg[MT_LY][MT_LX];
    __shared__ unsigned char sf[MT_LY][MT_LX];
    __shared__ double red[4][MT_TERMS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * MT_X, y0 = blockIdx.y * MT_Y;
    const size_t image = (size_t)blockIdx.z * H * W;

    for (int i = tid; i < MT_LY * MT_LX; i += 256) {
        const int ly = i / MT_LX, lx = i - ly * MT_LX;
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        float p = 0.0f, g = 0.0f;
        unsigned char f = 0;                   // outside the image: invalid, not finite
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t at = image + (size_t)y * W + x;
            p = pred[at];
            g = gt[at];
            const bool fin = isfinite(p) && isfinite(g);
            const bool ok = fin && p > 0.0f && g > 0.0f && (!mask_pred || mask_pred[at] > 0.5f) &&
                            (!mask_gt || mask_gt[at] > 0.5f);
            f = (unsigned char)((ok ? PIX_VALID : 0) | (fin ? PIX_FINITE : 0));
        }
        sp[ly][lx] = p;
        sg[ly][lx] = g;
        sf[ly][lx] = f;
    }
    __syncthreads();

    const int lx = (tid & 31) + 1, ly = (tid >> 5) + 1;
    const int x = x0 + lx - 1, y = y0 + ly - 1;
    double term[MT_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (x < W && y < H) {
        unsigned all9 = PIX_VALID;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) all9 &= sf[ly + dy][lx + dx];
        // the stencil of the normals: right, left, below, above; a border pixel has a neighbour outside the image
        const bool stencil = (sf[ly][lx + 1] & sf[ly][lx - 1] & sf[ly + 1][lx] & sf[ly - 1][lx] & PIX_FINITE) != 0;
        const bool counted = erode ? (all9 != 0) : ((sf[ly][lx] & PIX_VALID) != 0);
        if (counted) {
            const float p = sp[ly][lx], g = sg[ly][lx];
            const double d = (double)p - (double)g;
            const double delta = log((double)p) - log((double)g);
            term[0] = 1.0;
            term[1] = fabs(d);
            term[2] = d * d;
            term[3] = delta;
            term[4] = delta * delta;
            if (stencil) {
                const float *rr = rays + 3 * ((size_t)y * W + x + 1), *rl = rays + 3 * ((size_t)y * W + x - 1);
                const float *rb = rays + 3 * ((size_t)(y + 1) * W + x), *ra = rays + 3 * ((size_t)(y - 1) * W + x);
                const V3 np = normalize_eps(normal_raw(pt3_ray(sp[ly][lx + 1], rr), pt3_ray(sp[ly][lx - 1], rl),
                                                       pt3_ray(sp[ly + 1][lx], rb), pt3_ray(sp[ly - 1][lx], ra)));
                const V3 ng = normalize_eps(normal_raw(pt3_ray(sg[ly][lx + 1], rr), pt3_ray(sg[ly][lx - 1], rl),
                                                       pt3_ray(sg[ly + 1][lx], rb), pt3_ray(sg[ly - 1][lx], ra)));
                // the angle between them as atan2(|np x ng|, np . ng): the normals are unit only up to
                // NORMAL_EPS / |n| (1.3 % at 128 x 128, fov 10), which acos of the dot product would read as 13
                // degrees between identical depths; atan2 does not depend on the lengths
                const V3 c = cross3(np, ng);
                const float s = sqrtf(c.x * c.x + c.y * c.y + c.z * c.z);
                const float dot = np.x * ng.x + np.y * ng.y + np.z * ng.z;
                term[5] = 1.0;
                term[6] = (double)atan2f(s, dot);
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < MT_TERMS; k++) {
        const double v = wave_sum(term[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < MT_TERMS) {
        const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partials[tile * MT_TERMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

__global__ __launch_bounds__(64) void depth_metrics_finish(const double *__restrict__ partials, int tiles,
                                                          float *__restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double *p = partials + (size_t)b * tiles * MT_TERMS;
    double acc[MT_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = lane; t < tiles; t += 64)
#pragma unroll
        for (int k = 0; k < MT_TERMS; k++) acc[k] += p[(size_t)t * MT_TERMS + k];
#pragma unroll
    for (int k = 0; k < MT_TERMS; k++) acc[k] = wave_sum(acc[k]);
    if (lane != 0) return;
    float *o = out + (size_t)b * 5;
    const double n = acc[0];
    const float nan = __builtin_nanf("");
    o[0] = (float)n;
    if (n == 0.0) {
        o[1] = o[2] = o[3] = o[4] = nan;
        return;
    }
    const double mean = acc[3] / n;
    const double var = acc[4] / n - mean * mean;
    o[1] = (float)(acc[1] / n);
    o[2] = (float)(acc[2] / n);
    o[3] = (float)sqrt(var > 0.0 ? var : 0.0);
    o[4] = acc[5] > 0.0 ? (float)(acc[6] / acc[5] * (180.0 / 3.14159265358979323846)) : nan;
}

static size_t metrics_tiles(int H, int W) { return (size_t)cdiv(W, MT_X) * cdiv(H, MT_Y); }

}  // namespace g2s

using namespace g2s;

extern "C" size_t g2s_depth_metrics_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * metrics_tiles(H, W) * MT_TERMS * sizeof(double);
}

extern "C" int g2s_depth_metrics(const float *depth_pred, const float *depth_gt, const float *mask_pred,
                                 const float *mask_gt, const float *rays, int B, int H, int W, int erode, float *out,
                                 void *workspace, size_t workspace_bytes, g2s_stream_t stream) {
    G2S_REQUIRE(depth_pred && depth_gt && rays && out, "g2s_depth_metrics: NULL pointer");
    G2S_REQUIRE(B > 0 && B <= 65535, "g2s_depth_metrics: B = %d outside [1, 65535]", B);
    G2S_REQUIRE(H >= 3 && W >= 3 && H <= 32768 && W <= 32768, "g2s_depth_metrics: H = %d, W = %d outside [3, 32768]", H, W);
    const size_t need = g2s_depth_metrics_workspace_bytes(B, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(G2S_ERR_WORKSPACE, "g2s_depth_metrics: workspace of %zu bytes, %zu needed",
                    workspace ? workspace_bytes : (size_t)0, need);
    G2S_REQUIRE(((uintptr_t)workspace & 7) == 0, "g2s_depth_metrics: workspace must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    double *partials = (double *)workspace;
    depth_metrics_tiles<<<dim3(cdiv(W, MT_X), cdiv(H, MT_Y), B), 256, 0, st>>>(depth_pred, depth_gt, mask_pred, mask_gt,
                                                                             rays, H, W, erode, partials);
    depth_metrics_finish<<<B, 64, 0, st>>>(partials, (int)metrics_tiles(H, W), out);
    return check_launch("g2s_depth_metrics");
}
