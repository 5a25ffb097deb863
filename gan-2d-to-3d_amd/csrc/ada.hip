// ada.hip — the geometric and colour augmentation of adaptive discriminator augmentation (ADA):
// random_apply_affine + random_apply_color of stylegan2-pytorch/non_leaking.py, as two launches forward
// and two backward instead of the reference's chain (reflect pad, two 12-tap up passes, affine_grid,
// grid_sample at double resolution, two 12-tap stride-2 passes, colour matmul).
//
//   ada_up2            x [B,C,H,W] -> x2 [B,C,2Hp,2Wp], Hp = H+py0+py1, Wp = W+px0+px1: reflect padding indexed on
//                      the fly and the separable 2x SYM6 upsampling; the source patch and the row pass live in LDS.
//                      Per axis  x2[2m] = sum_j P[m+j-3] k[11-2j],  x2[2m+1] = sum_j P[m+j-2] k[10-2j]  (j = 0..5,
//                      P = the padded image, 0 outside it) — upfirdn(up 2, pad (6, 5)) with the zero taps dropped.
//   ada_warp_down      x2, Ginv [B,2,3], Cmat [B,3,4] or NULL -> y [B,C,H,W].  With A = grid_sample(x2,
//                      affine_grid(Ginv, [2(H+6), 2(W+6)]), bilinear, zeros, align_corners=False):
//                      y[n,m] = sum_{s,t} k[s] k[t] A[2n+1+s, 2m+1+t]   (upfirdn(down 2, flipped k, pad (-1,-1))),
//                      then y <- Cmat[:, :3] y + Cmat[:, 3] over the three channels.  A workgroup owns a 16x16 tile of
//                      y, evaluates A at the 42x42 positions it needs into LDS, runs both passes there and applies
//                      the colour matrix in the store: A and the row-pass intermediate never reach HBM.
//   ada_warp_down_bwd  gy -> gx2, the exact adjoint: a workgroup owns a 32x32 tile of A's gradient, gathers it from
//                      the 22x22 tile of (Cmat^T gy) that reaches it (6 taps per axis and parity) and scatters the
//                      bilinear adjoint with float atomics.
//   ada_down_bwd +     the same adjoint as a gather (g2s_ada_warp_down_bwd_gather): the first half of the above with
//   ada_warp_gather    A's gradient stored to a workspace, then one thread per gx2 element that walks the bounding
//                      box of the pre-image of its 2x2 neighbourhood under the affine map and sums, rows outer and
//                      columns inner, the forward's own bilinear weight times A's gradient.  No atomics, no clear.
//   ada_up2_bwd       gx2 -> gx, the exact adjoint: gP[q] = sum_u k[11-u] gx2[2q+6-u] per axis (a 12-tap stride-2
//                      pass), and gx[i] sums gP over the padded positions that reflect onto i — the direct one and up
//                      to one mirror image per side and axis.  Gathered per mirror image, no atomics.
//
// Ginv and Cmat get no gradient (the reference gives them none).
//
// Deterministic mode (g2s_set_deterministic): ada_warp_down_bwd scatters with float atomics whose order
// varies from run to run and has NO fixed-point variant — it REFUSES with G2S_ERR_INVALID while the mode is on.
// Every other kernel has one fixed summation order and runs in either mode with the same bits; the gather pair is
// the adjoint to call while the mode is on (augment.py's _AdaAdj reads the mode when it runs).
//
// Roofline class: the four fused kernels are HBM/L2-bound streaming passes with ~150-300 flops per output element from LDS;
// see DESIGN.md 4.20.
#include "g2s_common.h"

namespace g2s {

// sym6, 12 taps (PyWavelets' 'sym6' reconstruction low-pass, as tabulated in the ADA paper's code)
__constant__ float ADA_K[12] = {
    0.015404109327027373f, 0.0034907120842174702f, -0.11799011114819057f, -0.048311742585633f,
    0.4910559419267466f, 0.787641141030194f, 0.3379294217276218f, -0.07263752278646252f,
    -0.021060292512300564f, 0.04472490177066578f, 0.0017677118642428036f, -0.007800708325034148f};

struct AdaUp { int H, W, px0, py0, Hp, Wp; };

__device__ __forceinline__ int reflect(int i, int n) {   // one bounce: |pad| <= n - 1
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

constexpr int UP_R = 16, UP_C = 32;   // padded-image positions per workgroup: a 32 x 64 tile of x2

// grid (cdiv(Wp, 32), cdiv(Hp, 16), B*C)
__global__ __launch_bounds__(256) void ada_up2(const float *__restrict__ x, float *__restrict__ x2, AdaUp d) {
    // padded rows r0-3 .. r0+18: the even phase reaches 3 back, the odd phase 3 ahead
    __shared__ float src[UP_R + 6][UP_C + 6];
    __shared__ float mid[UP_R + 6][2 * UP_C + 1];
    const int tid = threadIdx.x, r0 = blockIdx.y * UP_R, c0 = blockIdx.x * UP_C;
    const float *xp = x + (size_t)blockIdx.z * d.H * d.W;
    for (int e = tid; e < (UP_R + 6) * (UP_C + 6); e += 256) {
        const int lr = e / (UP_C + 6), lc = e % (UP_C + 6), pr = r0 - 3 + lr, pc = c0 - 3 + lc;
        float v = 0.0f;
        if (pr >= 0 && pr < d.Hp && pc >= 0 && pc < d.Wp)
            v = xp[(size_t)reflect(pr - d.py0, d.H) * d.W + reflect(pc - d.px0, d.W)];
        src[lr][lc] = v;
    }
    __syncthreads();
    for (int e = tid; e < (UP_R + 6) * 2 * UP_C; e += 256) {
        const int lr = e / (2 * UP_C), o = e % (2 * UP_C), ml = o >> 1, ph = o & 1;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 6; j++) acc += src[lr][ml + j + ph] * ADA_K[11 - 2 * j - ph];
        mid[lr][o] = acc;
    }
    __syncthreads();
    const int H2 = 2 * d.Hp, W2 = 2 * d.Wp;
    float *yp = x2 + (size_t)blockIdx.z * H2 * W2;
    for (int e = tid; e < 2 * UP_R * 2 * UP_C; e += 256) {
        const int ro = e / (2 * UP_C), o = e % (2 * UP_C), ml = ro >> 1, ph = ro & 1;
        const int gr = 2 * r0 + ro, gc = 2 * c0 + o;
        if (gr >= H2 || gc >= W2) continue;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 6; j++) acc += mid[ml + j + ph][o] * ADA_K[11 - 2 * j - ph];
        yp[(size_t)gr * W2 + gc] = acc;
    }
}

// The padded positions that reflect onto image index i along one axis (pad p0 before, n samples, np padded):
// kind 0: p0 + i;  kind 1: p0 - i (1 <= i <= p0);  kind 2: p0 + 2(n-1) - i (i <= n-2, position < np).
// [lo, hi] = the indices of [i0, i1] that have an image of this kind (empty: lo > hi).
__device__ __forceinline__ int mirror_pos(int kind, int i, int p0, int n) {
    return kind == 0 ? p0 + i : (kind == 1 ? p0 - i : p0 + 2 * (n - 1) - i);
}
__device__ __forceinline__ void mirror_range(int kind, int i0, int i1, int p0, int n, int np, int &lo, int &hi) {
    lo = i0; hi = i1;
    if (kind == 1) { lo = max(lo, 1); hi = min(hi, p0); }
    if (kind == 2) { lo = max(lo, p0 + 2 * (n - 1) - (np - 1)); hi = min(hi, n - 2); }
}

constexpr int UB_T = 16;   // image positions per axis and workgroup

// grid (cdiv(W, 16), cdiv(H, 16), B*C)
__global__ __launch_bounds__(256) void ada_up2_bwd(const float *__restrict__ gx2, float *__restrict__ gx, AdaUp d) {
    __shared__ float g[2 * UB_T + 10][2 * UB_T + 11];
    __shared__ float mid[2 * UB_T + 10][UB_T + 1];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = blockIdx.y * UB_T, j0 = blockIdx.x * UB_T, i = i0 + ti, j = j0 + tj;
    const int i1 = min(i0 + UB_T, d.H) - 1, j1 = min(j0 + UB_T, d.W) - 1;
    const int H2 = 2 * d.Hp, W2 = 2 * d.Wp;
    const float *gp = gx2 + (size_t)blockIdx.z * H2 * W2;
    float acc = 0.0f;
    for (int kr = 0; kr < 3; kr++) {
        int rlo, rhi;
        mirror_range(kr, i0, i1, d.py0, d.H, d.Hp, rlo, rhi);
        if (rlo > rhi) continue;
        const int qr0 = min(mirror_pos(kr, rlo, d.py0, d.H), mirror_pos(kr, rhi, d.py0, d.H));
        for (int kc = 0; kc < 3; kc++) {
            int clo, chi;
            mirror_range(kc, j0, j1, d.px0, d.W, d.Wp, clo, chi);
            if (clo > chi) continue;
            const int qc0 = min(mirror_pos(kc, clo, d.px0, d.W), mirror_pos(kc, chi, d.px0, d.W));
            // rows 2 qr0 - 5 .. 2 qr0 + 36 of gx2 serve the padded rows qr0 .. qr0 + 15
            const int br = 2 * qr0 - 5, bc = 2 * qc0 - 5;
            __syncthreads();   // the previous image's reads of g and mid are done
            for (int e = tid; e < (2 * UB_T + 10) * (2 * UB_T + 10); e += 256) {
                const int lr = e / (2 * UB_T + 10), lc = e % (2 * UB_T + 10), r = br + lr, c = bc + lc;
                g[lr][lc] = (r >= 0 && r < H2 && c >= 0 && c < W2) ? gp[(size_t)r * W2 + c] : 0.0f;
            }
            __syncthreads();
            for (int e = tid; e < (2 * UB_T + 10) * UB_T; e += 256) {
                const int lr = e >> 4, tq = e & 15;
                float a = 0.0f;
#pragma unroll
                for (int u = 0; u < 12; u++) a += ADA_K[11 - u] * g[lr][2 * tq + 11 - u];
                mid[lr][tq] = a;
            }
            __syncthreads();
            if (i >= rlo && i <= rhi && j >= clo && j <= chi) {
                const int lqr = mirror_pos(kr, i, d.py0, d.H) - qr0, lqc = mirror_pos(kc, j, d.px0, d.W) - qc0;
                float a = 0.0f;
#pragma unroll
                for (int u = 0; u < 12; u++) a += ADA_K[11 - u] * mid[2 * lqr + 11 - u][lqc];
                acc += a;
            }
        }
    }
    if (i < d.H && j < d.W) gx[(size_t)blockIdx.z * d.H * d.W + (size_t)i * d.W + j] = acc;
}

struct AdaWarp { int C, H, W, H2, W2; };   // y [.., H, W], x2 [.., H2, W2]; A is 2(H+6) x 2(W+6)

struct Bilin {
    int x0, y0;
    float nw, ne, sw, se;
    bool in_x0, in_x1, in_y0, in_y1;
};

// A's sample (i, j): affine_grid's base point (align_corners=False), the affine map, grid_sample's
// un-normalisation (align_corners=False), the four corner weights in ATen's order.
__device__ __forceinline__ Bilin bilin_of(int i, int j, const float *t, const AdaWarp &d) {
    const int Hs = 2 * (d.H + 6), Ws = 2 * (d.W + 6);
    const float xs = (float)(2 * j + 1) / (float)Ws - 1.0f, ys = (float)(2 * i + 1) / (float)Hs - 1.0f;
    const float gx = t[0] * xs + t[1] * ys + t[2], gy = t[3] * xs + t[4] * ys + t[5];
    const float ix = ((gx + 1.0f) * (float)d.W2 - 1.0f) * 0.5f, iy = ((gy + 1.0f) * (float)d.H2 - 1.0f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    Bilin c;
    // a float outside the int range (or NaN) has no in-range corner, as in ATen
    const bool sane = fx >= -2.0f && fx <= (float)d.W2 && fy >= -2.0f && fy <= (float)d.H2;
    c.x0 = sane ? (int)fx : -2;
    c.y0 = sane ? (int)fy : -2;
    const float wx0 = (fx + 1.0f) - ix, wx1 = ix - fx, wy0 = (fy + 1.0f) - iy, wy1 = iy - fy;
    c.nw = wx0 * wy0; c.ne = wx1 * wy0; c.sw = wx0 * wy1; c.se = wx1 * wy1;
    c.in_x0 = c.x0 >= 0 && c.x0 < d.W2;
    c.in_x1 = c.x0 + 1 >= 0 && c.x0 + 1 < d.W2;
    c.in_y0 = c.y0 >= 0 && c.y0 < d.H2;
    c.in_y1 = c.y0 + 1 >= 0 && c.y0 + 1 < d.H2;
    return c;
}

constexpr int WD_T = 16, WD_S = 2 * WD_T + 10;   // output tile, A positions per axis

// grid (cdiv(W, 16), cdiv(H, 16), COLOR ? B : B*C).  COLOR: C == 3, the three channels in one workgroup.
template <bool COLOR>
__global__ __launch_bounds__(256) void ada_warp_down(const float *__restrict__ x2, const float *__restrict__ Ginv,
                                                     const float *__restrict__ Cmat, float *__restrict__ y, AdaWarp d) {
    __shared__ float a[WD_S][WD_S + 1];
    __shared__ float mid[WD_S][WD_T + 1];
    const int tid = threadIdx.x, tn = tid >> 4, tm = tid & 15;
    const int n0 = blockIdx.y * WD_T, m0 = blockIdx.x * WD_T;
    const int b = COLOR ? blockIdx.z : blockIdx.z / d.C, ch0 = COLOR ? 0 : blockIdx.z % d.C;
    const int Hs = 2 * (d.H + 6), Ws = 2 * (d.W + 6);
    float t[6];
#pragma unroll
    for (int q = 0; q < 6; q++) t[q] = Ginv[b * 6 + q];
    const size_t plane = (size_t)d.H2 * d.W2;
    float out[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int cc = 0; cc < (COLOR ? 3 : 1); cc++) {
        const float *xp = x2 + ((size_t)b * d.C + ch0 + cc) * plane;
        if (cc) __syncthreads();   // the previous channel's reads of a and mid are done
        for (int e = tid; e < WD_S * WD_S; e += 256) {
            const int lr = e / WD_S, lc = e % WD_S, i = 2 * n0 + 1 + lr, j = 2 * m0 + 1 + lc;
            float v = 0.0f;
            if (i < Hs && j < Ws) {
                const Bilin c = bilin_of(i, j, t, d);
                const float *p = xp + (long)c.y0 * d.W2 + c.x0;   // only dereferenced for in-range corners
                if (c.in_y0 && c.in_x0) v += p[0] * c.nw;
                if (c.in_y0 && c.in_x1) v += p[1] * c.ne;
                if (c.in_y1 && c.in_x0) v += p[d.W2] * c.sw;
                if (c.in_y1 && c.in_x1) v += p[d.W2 + 1] * c.se;
            }
            a[lr][lc] = v;
        }
        __syncthreads();
        for (int e = tid; e < WD_S * WD_T; e += 256) {
            const int lr = e >> 4, m = e & 15;
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 12; q++) acc += ADA_K[q] * a[lr][2 * m + q];
            mid[lr][m] = acc;
        }
        __syncthreads();
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 12; q++) acc += ADA_K[q] * mid[2 * tn + q][tm];
        out[cc] = acc;
    }
    const int n = n0 + tn, m = m0 + tm;
    if (n >= d.H || m >= d.W) return;
    const size_t hw = (size_t)d.H * d.W;
    float *yp = y + ((size_t)b * d.C + ch0) * hw + (size_t)n * d.W + m;
    if (COLOR) {
        const float *cm = Cmat + b * 12;
#pragma unroll
        for (int c = 0; c < 3; c++)
            yp[c * hw] = cm[c * 4] * out[0] + cm[c * 4 + 1] * out[1] + cm[c * 4 + 2] * out[2] + cm[c * 4 + 3];
    } else {
        yp[0] = out[0];
    }
}

constexpr int WB_T = 32, WB_G = WB_T / 2 + 6;   // A positions per axis and workgroup, gy positions that reach them

// grid (cdiv(Ws, 32), cdiv(Hs, 32), COLOR ? B : B*C); gx2 zero-filled by the launcher
template <bool COLOR>
__global__ __launch_bounds__(256) void ada_warp_down_bwd(const float *__restrict__ gy, const float *__restrict__ Ginv,
                                                         const float *__restrict__ Cmat, float *__restrict__ gx2,
                                                         AdaWarp d) {
    __shared__ float gz[WB_G][WB_G + 1];
    __shared__ float tmp[WB_T][WB_G + 1];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * WB_T, j0 = blockIdx.x * WB_T, nb = i0 / 2 - 6, mb = j0 / 2 - 6;
    const int b = COLOR ? blockIdx.z : blockIdx.z / d.C, ch0 = COLOR ? 0 : blockIdx.z % d.C;
    const int Hs = 2 * (d.H + 6), Ws = 2 * (d.W + 6);
    float t[6];
#pragma unroll
    for (int q = 0; q < 6; q++) t[q] = Ginv[b * 6 + q];
    const size_t plane = (size_t)d.H2 * d.W2, hw = (size_t)d.H * d.W;
    for (int cc = 0; cc < (COLOR ? 3 : 1); cc++) {
        if (cc) __syncthreads();
        for (int e = tid; e < WB_G * WB_G; e += 256) {
            const int ln = e / WB_G, lm = e % WB_G, n = nb + ln, m = mb + lm;
            float v = 0.0f;
            if (n >= 0 && n < d.H && m >= 0 && m < d.W) {
                const float *gp = gy + (size_t)b * d.C * hw + (size_t)n * d.W + m;
                if (COLOR) {   // the transposed colour matrix: column cc
                    const float *cm = Cmat + b * 12 + cc;
                    v = cm[0] * gp[0] + cm[4] * gp[hw] + cm[8] * gp[2 * hw];
                } else {
                    v = gp[ch0 * hw];
                }
            }
            gz[ln][lm] = v;
        }
        __syncthreads();
        // A row i takes tap s = i - 1 - 2n of gy row n: the six s of i's parity
        for (int e = tid; e < WB_T * WB_G; e += 256) {
            const int li = e / WB_G, lm = e % WB_G, s0 = (li & 1) ? 0 : 1;
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const int s = s0 + 2 * q;
                acc += ADA_K[s] * gz[(li - 1 - s) / 2 + 6][lm];
            }
            tmp[li][lm] = acc;
        }
        __syncthreads();
        float *xp = gx2 + ((size_t)b * d.C + ch0 + cc) * plane;
        for (int e = tid; e < WB_T * WB_T; e += 256) {
            const int li = e >> 5, lj = e & 31, i = i0 + li, j = j0 + lj, s0 = (lj & 1) ? 0 : 1;
            if (i >= Hs || j >= Ws) continue;
            float ga = 0.0f;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const int s = s0 + 2 * q;
                ga += ADA_K[s] * tmp[li][(lj - 1 - s) / 2 + 6];
            }
            if (ga == 0.0f) continue;   // outside the support of gy: nothing to add
            const Bilin c = bilin_of(i, j, t, d);
            float *p = xp + (long)c.y0 * d.W2 + c.x0;
            if (c.in_y0 && c.in_x0) unsafeAtomicAdd(p, c.nw * ga);
            if (c.in_y0 && c.in_x1) unsafeAtomicAdd(p + 1, c.ne * ga);
            if (c.in_y1 && c.in_x0) unsafeAtomicAdd(p + d.W2, c.sw * ga);
            if (c.in_y1 && c.in_x1) unsafeAtomicAdd(p + d.W2 + 1, c.se * ga);
        }
    }
}

// The first half of ada_warp_down_bwd (Cmat^T gy, then the two 6-taps-per-parity passes) with A's gradient stored:
// ga [B, C, Hs, Ws], every element written exactly once.  Same tiling, same order of operations.
// grid (cdiv(Ws, 32), cdiv(Hs, 32), COLOR ? B : B*C)
template <bool COLOR>
__global__ __launch_bounds__(256) void ada_down_bwd(const float *__restrict__ gy, const float *__restrict__ Cmat,
                                                    float *__restrict__ ga_out, AdaWarp d) {
    __shared__ float gz[WB_G][WB_G + 1];
    __shared__ float tmp[WB_T][WB_G + 1];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * WB_T, j0 = blockIdx.x * WB_T, nb = i0 / 2 - 6, mb = j0 / 2 - 6;
    const int b = COLOR ? blockIdx.z : blockIdx.z / d.C, ch0 = COLOR ? 0 : blockIdx.z % d.C;
    const int Hs = 2 * (d.H + 6), Ws = 2 * (d.W + 6);
    const size_t hw = (size_t)d.H * d.W;
    for (int cc = 0; cc < (COLOR ? 3 : 1); cc++) {
        if (cc) __syncthreads();
        for (int e = tid; e < WB_G * WB_G; e += 256) {
            const int ln = e / WB_G, lm = e % WB_G, n = nb + ln, m = mb + lm;
            float v = 0.0f;
            if (n >= 0 && n < d.H && m >= 0 && m < d.W) {
                const float *gp = gy + (size_t)b * d.C * hw + (size_t)n * d.W + m;
                if (COLOR) {
                    const float *cm = Cmat + b * 12 + cc;
                    v = cm[0] * gp[0] + cm[4] * gp[hw] + cm[8] * gp[2 * hw];
                } else {
                    v = gp[ch0 * hw];
                }
            }
            gz[ln][lm] = v;
        }
        __syncthreads();
        for (int e = tid; e < WB_T * WB_G; e += 256) {
            const int li = e / WB_G, lm = e % WB_G, s0 = (li & 1) ? 0 : 1;
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const int s = s0 + 2 * q;
                acc += ADA_K[s] * gz[(li - 1 - s) / 2 + 6][lm];
            }
            tmp[li][lm] = acc;
        }
        __syncthreads();
        float *ap = ga_out + ((size_t)b * d.C + ch0 + cc) * Hs * Ws;
        for (int e = tid; e < WB_T * WB_T; e += 256) {
            const int li = e >> 5, lj = e & 31, i = i0 + li, j = j0 + lj, s0 = (lj & 1) ? 0 : 1;
            if (i >= Hs || j >= Ws) continue;
            float ga = 0.0f;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const int s = s0 + 2 * q;
                ga += ADA_K[s] * tmp[li][(lj - 1 - s) / 2 + 6];
            }
            ap[(size_t)i * Ws + j] = ga;
        }
    }
}

constexpr int GA_TX = 32, GA_TY = 8;   // gx2 positions per workgroup

// The bilinear adjoint as a gather: one thread per gx2[b, c, sy, sx], one fixed summation order, no atomics.
//
// In exact arithmetic bilin_of's sample position is affine in A's position (i, j):
//   ix = jxx j + jxy i + ox,   iy = jyx j + jyy i + oy,
//   jxx = t0 W2 / Ws, jxy = t1 W2 / Hs, jyx = t3 H2 / Ws, jyy = t4 H2 / Hs.
// A's position (i, j) has (sy, sx) among its four corners only if |ix - sx| < 1 and |iy - sy| < 1.  bilin_of
// computes ix in float32: four roundings of values no larger than about (|t0| + |t1| + |t2| + 1) W2, hence the
// slack `sl` on the square's half side (4 ulp of that magnitude, 1.2e-7 each).  The pre-image of the square
// under the inverse Jacobian is a parallelogram; its bounding box, widened by one position per side and clipped
// to A, holds every candidate.  The weight of a candidate comes from bilin_of itself — the forward's own float32
// weights, so this is the transpose of what the forward applies — and a candidate whose corners miss (sy, sx)
// adds nothing.  A singular or near-singular matrix (or a non-finite one) makes the box all of A: slow, and
// neither wrong nor unbounded.  The box is computed in double: at sides of 32768 a float32 pre-image would
// itself be off by more than the one position of widening.
// grid (cdiv(W2, 32), cdiv(H2, 8), B*C)
__global__ __launch_bounds__(256) void ada_warp_gather(const float *__restrict__ ga, const float *__restrict__ Ginv,
                                                       float *__restrict__ gx2, AdaWarp d) {
    __shared__ double inv[8];   // inverse Jacobian (4), offsets ox, oy, half extents of the box in j and i
    const int tid = threadIdx.x;
    const int b = blockIdx.z / d.C;
    const int Hs = 2 * (d.H + 6), Ws = 2 * (d.W + 6);
    float t[6];
#pragma unroll
    for (int q = 0; q < 6; q++) t[q] = Ginv[b * 6 + q];
    if (tid == 0) {
        const double w2 = d.W2, h2 = d.H2, ws = Ws, hs = Hs;
        const double jxx = t[0] * w2 / ws, jxy = t[1] * w2 / hs, jyx = t[3] * h2 / ws, jyy = t[4] * h2 / hs;
        const double ox = ((t[0] * (1.0 / ws - 1.0) + t[1] * (1.0 / hs - 1.0) + t[2] + 1.0) * w2 - 1.0) * 0.5;
        const double oy = ((t[3] * (1.0 / ws - 1.0) + t[4] * (1.0 / hs - 1.0) + t[5] + 1.0) * h2 - 1.0) * 0.5;
        const double det = jxx * jyy - jxy * jyx;
        const double slx = 1.0 + 4.8e-7 * (fabs((double)t[0]) + fabs((double)t[1]) + fabs((double)t[2]) + 1.0) * w2;
        const double sly = 1.0 + 4.8e-7 * (fabs((double)t[3]) + fabs((double)t[4]) + fabs((double)t[5]) + 1.0) * h2;
        // [j; i] = inv ([ix; iy] - [ox; oy])
        const double a = jyy / det, bb = -jxy / det, c = -jyx / det, dd = jxx / det;
        inv[0] = a; inv[1] = bb; inv[2] = c; inv[3] = dd; inv[4] = ox; inv[5] = oy;
        inv[6] = fabs(a) * slx + fabs(bb) * sly + 1.0;
        inv[7] = fabs(c) * slx + fabs(dd) * sly + 1.0;
    }
    __syncthreads();
    const int sx = blockIdx.x * GA_TX + (tid & (GA_TX - 1)), sy = blockIdx.y * GA_TY + tid / GA_TX;
    if (sx >= d.W2 || sy >= d.H2) return;
    int jlo = 0, jhi = Ws - 1, ilo = 0, ihi = Hs - 1;
    const double ej = inv[6], ei = inv[7];
    const double rx = (double)sx - inv[4], ry = (double)sy - inv[5];
    const double pj = inv[0] * rx + inv[1] * ry, pi = inv[2] * rx + inv[3] * ry;
    // anything non-finite or wider than A fails these tests and keeps the whole range
    if (ej < (double)Ws && fabs(pj) < 1e9) {
        jlo = (int)fmax(floor(pj - ej), 0.0);
        jhi = (int)fmin(ceil(pj + ej), (double)(Ws - 1));
    }
    if (ei < (double)Hs && fabs(pi) < 1e9) {
        ilo = (int)fmax(floor(pi - ei), 0.0);
        ihi = (int)fmin(ceil(pi + ei), (double)(Hs - 1));
    }
    const float *ap = ga + (size_t)blockIdx.z * Hs * Ws;
    float acc = 0.0f;
    for (int i = ilo; i <= ihi; i++) {
        for (int j = jlo; j <= jhi; j++) {
            const Bilin c = bilin_of(i, j, t, d);
            const int dx = sx - c.x0, dy = sy - c.y0;
            if ((dx | dy) & ~1) continue;   // (sy, sx) is none of the four corners
            const bool in_x = dx ? c.in_x1 : c.in_x0, in_y = dy ? c.in_y1 : c.in_y0;
            if (!(in_x && in_y)) continue;
            const float w = dy ? (dx ? c.se : c.sw) : (dx ? c.ne : c.nw);
            acc += __fmul_rn(w, ap[(size_t)i * Ws + j]);   // the scatter's product, rounded before it is added
        }
    }
    gx2[(size_t)blockIdx.z * d.H2 * d.W2 + (size_t)sy * d.W2 + sx] = acc;
}

static int up_check(const char *what, int B, int C, int H, int W, int px0, int px1, int py0, int py1) {
    G2S_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "%s: sizes must be positive", what);
    G2S_REQUIRE(px0 >= 0 && px1 >= 0 && py0 >= 0 && py1 >= 0, "%s: pads must be non-negative", what);
    G2S_REQUIRE(px0 <= W - 1 && px1 <= W - 1 && py0 <= H - 1 && py1 <= H - 1,
                "%s: reflect padding needs pad <= size - 1 (pads %d %d %d %d on %d x %d)", what, px0, px1, py0, py1, H, W);
    G2S_REQUIRE((long)B * C <= 65535 && H <= (1 << 14) && W <= (1 << 14), "%s: B*C <= 65535, sides <= 16384", what);
    return G2S_OK;
}

static int warp_check(const char *what, const float *Cmat, int B, int C, int H, int W, int H2, int W2) {
    G2S_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && H2 > 0 && W2 > 0, "%s: sizes must be positive", what);
    G2S_REQUIRE(!Cmat || C == 3, "%s: a colour matrix needs C == 3 (got %d)", what, C);
    G2S_REQUIRE((long)B * C <= 65535 && H <= (1 << 14) && W <= (1 << 14) && H2 <= (1 << 15) && W2 <= (1 << 15),
                "%s: B*C <= 65535, sides <= 16384 (x2: 32768)", what);
    return G2S_OK;
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_ada_up2(const float *x, float *x2, int B, int C, int H, int W, int px0, int px1, int py0, int py1,
                           g2s_stream_t stream) {
    G2S_REQUIRE(x && x2, "g2s_ada_up2: NULL pointer argument");
    int rc = up_check("g2s_ada_up2", B, C, H, W, px0, px1, py0, py1);
    if (rc) return rc;
    const AdaUp d{H, W, px0, py0, H + py0 + py1, W + px0 + px1};
    ada_up2<<<dim3(cdiv(d.Wp, UP_C), cdiv(d.Hp, UP_R), B * C), 256, 0, as_stream(stream)>>>(x, x2, d);
    return check_launch("g2s_ada_up2");
}

extern "C" int g2s_ada_up2_bwd(const float *gx2, float *gx, int B, int C, int H, int W, int px0, int px1, int py0,
                               int py1, g2s_stream_t stream) {
    G2S_REQUIRE(gx2 && gx, "g2s_ada_up2_bwd: NULL pointer argument");
    int rc = up_check("g2s_ada_up2_bwd", B, C, H, W, px0, px1, py0, py1);
    if (rc) return rc;
    const AdaUp d{H, W, px0, py0, H + py0 + py1, W + px0 + px1};
    ada_up2_bwd<<<dim3(cdiv(W, UB_T), cdiv(H, UB_T), B * C), 256, 0, as_stream(stream)>>>(gx2, gx, d);
    return check_launch("g2s_ada_up2_bwd");
}

extern "C" int g2s_ada_warp_down(const float *x2, const float *Ginv, const float *Cmat, float *y, int B, int C, int H,
                                 int W, int H2, int W2, g2s_stream_t stream) {
    G2S_REQUIRE(x2 && Ginv && y, "g2s_ada_warp_down: NULL pointer argument (only Cmat may be NULL)");
    int rc = warp_check("g2s_ada_warp_down", Cmat, B, C, H, W, H2, W2);
    if (rc) return rc;
    const AdaWarp d{C, H, W, H2, W2};
    const dim3 g(cdiv(W, WD_T), cdiv(H, WD_T), Cmat ? B : B * C);
    if (Cmat) ada_warp_down<true><<<g, 256, 0, as_stream(stream)>>>(x2, Ginv, Cmat, y, d);
    else ada_warp_down<false><<<g, 256, 0, as_stream(stream)>>>(x2, Ginv, nullptr, y, d);
    return check_launch("g2s_ada_warp_down");
}

extern "C" int g2s_ada_warp_down_bwd(const float *gy, const float *Ginv, const float *Cmat, float *gx2, int B, int C,
                                     int H, int W, int H2, int W2, int acc_is_zero, g2s_stream_t stream) {
    G2S_REQUIRE(gy && Ginv && gx2, "g2s_ada_warp_down_bwd: NULL pointer argument (only Cmat may be NULL)");
    int rc = warp_check("g2s_ada_warp_down_bwd", Cmat, B, C, H, W, H2, W2);
    if (rc) return rc;
    G2S_REQUIRE(!deterministic(), "g2s_ada_warp_down_bwd: float-atomic scatter, no deterministic variant "
                                  "(switch the mode off for the augmentation's backward)");
    hipStream_t st = as_stream(stream);
    if (!acc_is_zero && hipMemsetAsync(gx2, 0, (size_t)B * C * H2 * W2 * sizeof(float), st) != hipSuccess)
        return fail(G2S_ERR_LAUNCH, "g2s_ada_warp_down_bwd: hipMemsetAsync(gx2) failed");
    const AdaWarp d{C, H, W, H2, W2};
    const dim3 g(cdiv(2 * (W + 6), WB_T), cdiv(2 * (H + 6), WB_T), Cmat ? B : B * C);
    if (Cmat) ada_warp_down_bwd<true><<<g, 256, 0, as_stream(stream)>>>(gy, Ginv, Cmat, gx2, d);
    else ada_warp_down_bwd<false><<<g, 256, 0, as_stream(stream)>>>(gy, Ginv, nullptr, gx2, d);
    return check_launch("g2s_ada_warp_down_bwd");
}

extern "C" int g2s_ada_warp_down_bwd_gather(const float *gy, const float *Ginv, const float *Cmat, float *gx2,
                                            float *ga, int B, int C, int H, int W, int H2, int W2,
                                            g2s_stream_t stream) {
    G2S_REQUIRE(gy && Ginv && gx2 && ga, "g2s_ada_warp_down_bwd_gather: NULL pointer argument (only Cmat may be NULL)");
    int rc = warp_check("g2s_ada_warp_down_bwd_gather", Cmat, B, C, H, W, H2, W2);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const AdaWarp d{C, H, W, H2, W2};
    const dim3 g1(cdiv(2 * (W + 6), WB_T), cdiv(2 * (H + 6), WB_T), Cmat ? B : B * C);
    if (Cmat) ada_down_bwd<true><<<g1, 256, 0, st>>>(gy, Cmat, ga, d);
    else ada_down_bwd<false><<<g1, 256, 0, st>>>(gy, nullptr, ga, d);
    rc = check_launch("g2s_ada_warp_down_bwd_gather (down)");
    if (rc) return rc;
    ada_warp_gather<<<dim3(cdiv(W2, GA_TX), cdiv(H2, GA_TY), B * C), 256, 0, st>>>(ga, Ginv, gx2, d);
    return check_launch("g2s_ada_warp_down_bwd_gather");
}
