// canon_mask.hip — the object mask of the input image carried into the canonical frame (model.py forward_step1 with
// object_mask on; Renderer.canon_mask):
//
//   grid       = get_warped_2d_grid(depth)          canonical pixel -> its position in the input image, [-1, 1]
//   canon_mask = grid_sample(mask, grid, bilinear, zeros padding, align_corners=True)
//
// as ONE launch per call: per canonical pixel  d * ray -> R (X - c) + c + t -> / z -> K -> [-1, 1] -> four mask taps ->
// one store.  The composed route spends about ten launches and a [B,S,S,3] and a [B,S,S,2] intermediate on it.
//
// No gradient (the mask is data), no atomics, no LDS, no workspace: every output element is written by exactly one
// thread from inputs alone, so the result is bit-identical from run to run in every mode.  The arithmetic restates the
// composition operation by operation (warp_verts_fwd of geometry.hip, then grid_3d_to_2d of renderer.py, then ATen's
// GridSampler as grid_sample.hip states it); the file is built with -ffp-contract=off so that no step contracts to an FMA
// the composition does not have.
#include "g2s_common.h"

namespace g2s {

struct CmIntr { float k00, k01, k02, k10, k11, k12, wm1, hm1; };  // wm1 = W - 1, hm1 = H - 1

// grid (ceil(H*W / 256), B); mask [Bm, H, W] with Bm in {1, B}; out [B, H, W]
__global__ __launch_bounds__(256) void canon_mask_kernel(const float *__restrict__ depth, const float *__restrict__ rays,
                                                         const float *__restrict__ R, const float *__restrict__ t, float rcd,
                                                         CmIntr K, const float *__restrict__ mask, float *__restrict__ out,
                                                         int H, int W, int Bm) {
    const int P = H * W;
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float *r = R + b * 9, *tt = t + b * 3;
    const float d = depth[(size_t)b * P + p];
    // X = d * ray - c;  Y = R X + c + t  (warp_verts_fwd)
    const float x = rays[3 * p] * d, y = rays[3 * p + 1] * d, z = rays[3 * p + 2] * d - rcd;
    const float yx = (x * r[0] + y * r[1] + z * r[2]) + tt[0];
    const float yy = (x * r[3] + y * r[4] + z * r[5]) + tt[1];
    const float yz = ((x * r[6] + y * r[7] + z * r[8]) + rcd) + tt[2];
    // projection and normalisation (grid_3d_to_2d): (Y / Y.z) K^T, then / (W - 1, H - 1) * 2 - 1
    const float a = yx / yz, bq = yy / yz;
    const float u = (a * K.k00 + bq * K.k01) + K.k02, v = (a * K.k10 + bq * K.k11) + K.k12;
    const float gx = u / K.wm1 * 2.0f - 1.0f, gy = v / K.hm1 * 2.0f - 1.0f;
    // bilinear read, zeros padding, align_corners=True (grid_sample.hip corner_of / grid_sample_fwd)
    const float ix = ((gx + 1.0f) / 2.0f) * K.wm1, iy = ((gy + 1.0f) / 2.0f) * K.hm1;
    const float fx = floorf(ix), fy = floorf(iy);
    // a position outside the int range (or NaN, a vertex on the camera plane) has no in-range tap and reads nothing
    const bool sane = fx >= -2.0f && fx <= (float)W && fy >= -2.0f && fy <= (float)H;
    const int x0 = sane ? (int)fx : -2, y0 = sane ? (int)fy : -2;
    const float wx0 = (fx + 1.0f) - ix, wx1 = ix - fx, wy0 = (fy + 1.0f) - iy, wy1 = iy - fy;
    const bool in_x0 = x0 >= 0 && x0 < W, in_x1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool in_y0 = y0 >= 0 && y0 < H, in_y1 = y0 + 1 >= 0 && y0 + 1 < H;
    const float *m = mask + (size_t)(Bm == 1 ? 0 : b) * P;
    float o = 0.0f;
    if (in_y0 && in_x0) o += m[y0 * W + x0] * (wx0 * wy0);
    if (in_y0 && in_x1) o += m[y0 * W + x0 + 1] * (wx1 * wy0);
    if (in_y1 && in_x0) o += m[(y0 + 1) * W + x0] * (wx0 * wy1);
    if (in_y1 && in_x1) o += m[(y0 + 1) * W + x0 + 1] * (wx1 * wy1);
    out[(size_t)b * P + p] = o;
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_canon_mask(const float *depth, const float *rays, const float *R, const float *t, const float *K,
                              float rot_center_depth, const float *mask, float *out, int B, int Bm, int H, int W,
                              g2s_stream_t stream) {
    G2S_REQUIRE(depth && rays && R && t && K && mask && out, "NULL pointer argument");
    G2S_REQUIRE(B > 0 && B <= 65535 && H > 1 && W > 1 && (long)H * W < (1L << 30), "bad size (B in 1..65535, H, W >= 2)");
    G2S_REQUIRE(Bm == 1 || Bm == B, "mask batch must be 1 or B");
    const CmIntr k{K[0], K[1], K[2], K[3], K[4], K[5], (float)(W - 1), (float)(H - 1)};
    canon_mask_kernel<<<dim3(cdiv((long)H * W, 256), B), 256, 0, as_stream(stream)>>>(depth, rays, R, t, rot_center_depth, k,
                                                                                    mask, out, H, W, Bm);
    return check_launch("g2s_canon_mask");
}
