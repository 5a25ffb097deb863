// sweep.hip — the viewing path: V poses of the same depth mesh per image in three launches (Renderer.render_sweep):
// g2s_sweep_verts, g2s_raster_depth_fwd over the B*V posed meshes, g2s_sweep_shade.  The loop it stands beside
// (Renderer._sweep) rebuilds the texture cubes of the whole image and runs its own rotate / rasterise / texture
// pass per pose; here the image and the normals are read in place as per-vertex attributes that all V frames of
// an image share, and the shading of GAN2Shape/model.py:355-358 (get_shading) is applied in the same pass.
//
//   sweep_verts_kernel<W>   out[b*V + v, n] = A[b,v] . verts[b,n] + t[b,v].  A streaming write of B*V*N*3 floats.
//                           A thread owns W consecutive floats of the flat [N*3] row (W = 4: one 16-byte store per
//                           frame; W = 1 when N*3 is no multiple of 4).  The two (one) vertices those floats belong
//                           to are loaded ONCE into registers and reused for the SWEEP_VPB frames of the block; the
//                           twelve pose values of a frame are wave-uniform loads.  Grid (floats / W / 256, V /
//                           SWEEP_VPB, B): the frames of an image are spread over the grid so that B = 1 fills the
//                           device too, the re-read of the vertices by the other frame groups hits L2.
//   sweep_shade_kernel      one thread per output pixel, as raster_rgb_kernel (the same resolve_pixel and
//                           persp_weights of shade_core.h, the same winner_verts): per supersample the winner's three
//                           vertices, perspective-correct weights u_k = w_k D / z_k (D = 1 / sum w_k / z_k, z of the
//                           POSED vertices; no clamp, no renormalisation), attribute and normal gathered at the
//                           vertices from the maps of image b = f / V (a few hundred KB, resident in L2 for all V
//                           frames), then the mode's colour; flip + ssaa x ssaa average and alpha as
//                           g2s_raster_rgba_fwd.  No atomics: bit-identical from run to run.
//
// The pseudo-view path (Renderer.render_pseudo_sweep) shares the first two launches and ends in
//   sweep_pseudo_kernel     the inverse-warp renderer the offset encoder was trained on (render_given_view with
//                           grid_sample=True after the relighting of sample_pseudo_imgs) for B*V frames at once: per
//                           output pixel the clamp of warp_canon_depth, the inverse of the frame's pose, K, the
//                           bilinear read of the RELIT canonical image and the nearest read of the canonical mask.
//                           The relit image is never formed: the four taps are shaded from the albedo and the normals
//                           of image b = f / V (6 S^2 floats, resident in L2 for all V frames) and then interpolated,
//                           which is "shade, then grid_sample" tap for tap.  One thread per output pixel, a workgroup
//                           lies inside one frame, so pose and light are wave-uniform loads; gather- and latency-
//                           bound, the stores are coalesced rows of a plane.  No atomics.
// No backward: nothing here carries a gradient.
#include "g2s_common.h"
#include "raster_core.h"
#include "shade_core.h"

namespace g2s {

constexpr int SWEEP_VPB = 8;   // frames per workgroup of sweep_verts_kernel

template <int W>
__global__ __launch_bounds__(256) void sweep_verts_kernel(const float *__restrict__ verts,
                                                          const float *__restrict__ pose, float *__restrict__ out,
                                                          int V, long row) {   // row = N * 3 floats
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * W;
    if (j0 >= row) return;
    const int b = blockIdx.z;
    const long n0 = j0 / 3;
    constexpr int NV = W == 1 ? 1 : 2;            // vertices that W consecutive floats touch (W <= 4)
    const long nlast = (j0 + W - 1) / 3;
    float p[NV][3];
    const float *src = verts + (size_t)b * row;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const long n = n0 + i <= nlast ? n0 + i : nlast;
#pragma unroll
        for (int k = 0; k < 3; k++) p[i][k] = src[n * 3 + k];
    }
    int which[W], comp[W];
#pragma unroll
    for (int i = 0; i < W; i++) {
        const long n = (j0 + i) / 3;
        which[i] = (int)(n - n0);
        comp[i] = (int)(j0 + i - n * 3);
    }
    const int v0 = blockIdx.y * SWEEP_VPB, v1 = min(V, v0 + SWEEP_VPB);
    for (int v = v0; v < v1; v++) {
        const float *q = pose + ((size_t)b * V + v) * 12;     // wave-uniform
        float o[W];
#pragma unroll
        for (int i = 0; i < W; i++) {
            const float x = which[i] ? p[NV - 1][0] : p[0][0];
            const float y = which[i] ? p[NV - 1][1] : p[0][1];
            const float z = which[i] ? p[NV - 1][2] : p[0][2];
            const int c = comp[i];
            const float a0 = c == 0 ? q[0] : c == 1 ? q[3] : q[6];
            const float a1 = c == 0 ? q[1] : c == 1 ? q[4] : q[7];
            const float a2 = c == 0 ? q[2] : c == 1 ? q[5] : q[8];
            const float t = c == 0 ? q[9] : c == 1 ? q[10] : q[11];
            o[i] = ((a0 * x + a1 * y) + a2 * z) + t;
        }
        float *dst = out + ((size_t)b * V + v) * row + j0;
        if (W == 4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[W > 1 ? 1 : 0], o[W > 2 ? 2 : 0], o[W > 3 ? 3 : 0]);
        } else {
#pragma unroll
            for (int i = 0; i < W; i++) dst[i] = o[i];
        }
    }
}

struct ShadeParams {
    const float *verts;      // [B*V, N, 3] posed
    const int32_t *faces;    // [F, 3] or NULL (implicit regular grid)
    const int32_t *face_idx; // [B*V, is, is]
    const float *bary;       // [B*V, is, is, 3]
    const float *attr;       // [B, C, N] or NULL
    const float *normal;     // [B, N, 3] or NULL
    const float *pose;       // [B, V, 12] or NULL
    const float *light;      // [B*V, 5] or NULL
    float *out;              // [B*V, Cout, S, S]
    float *alpha;            // [B*V, S, S] or NULL
    int B, V, N, F, S, is, ssaa, C, Cout, fill_back;
    float grey;
    float bg[4];
};

// Colour of one supersample of frame f.  Returns whether the sample has a winner.
template <bool IMPLICIT, int MODE>
__device__ __forceinline__ bool shade_sample(const ShadeParams &p, int f, int b, int yi, int xi, float col[4]) {
    const size_t si = ((size_t)f * p.is + yi) * p.is + xi;
    const int fn = p.face_idx[si];
    if (fn < 0) {
        for (int c = 0; c < p.Cout; c++) col[c] = p.bg[c];
        return false;
    }
    int g, v[3];
    bool rev;
    winner_verts(fn, p.F, p.S, IMPLICIT ? nullptr : p.faces, p.fill_back, g, rev, v);
    float w[3], z[3], wz[3], u[3];
    for (int k = 0; k < 3; k++) {
        w[k] = p.bary[3 * si + k];
        z[k] = p.verts[((size_t)f * p.N + v[k]) * 3 + 2];
    }
    const float depth = persp_weights(w, z, wz);
    for (int k = 0; k < 3; k++) u[k] = w[k] * depth / z[k];
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (MODE == 0 || MODE == 1) {
        for (int c = 0; c < p.C; c++) {
            const float *src = p.attr + ((size_t)b * p.C + c) * p.N;
            a[c] = (u[0] * src[v[0]] + u[1] * src[v[1]]) + u[2] * src[v[2]];
        }
    }
    if (MODE == 0) {
        for (int c = 0; c < p.C; c++) col[c] = a[c];
        return true;
    }
    const float *nm = p.normal + (size_t)b * p.N * 3;
    float m[3], n[3];
    for (int c = 0; c < 3; c++)
        m[c] = (u[0] * nm[(size_t)v[0] * 3 + c] + u[1] * nm[(size_t)v[1] * 3 + c]) + u[2] * nm[(size_t)v[2] * 3 + c];
    const float *A = p.pose + ((size_t)f) * 12;   // f = b*V + v indexes [B, V, 12] directly
    for (int c = 0; c < 3; c++) n[c] = (A[3 * c] * m[0] + A[3 * c + 1] * m[1]) + A[3 * c + 2] * m[2];
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float den = fmaxf(len, 1e-12f);
    for (int c = 0; c < 3; c++) n[c] = n[c] / den;
    if (MODE == 3) {
        for (int c = 0; c < 3; c++) col[c] = n[c];
        return true;
    }
    const float *l = p.light + (size_t)f * 5;
    const float dot = (n[0] * l[2] + n[1] * l[3]) + n[2] * l[4];
    const float shade = l[0] + l[1] * fmaxf(dot, 0.0f);
    if (MODE == 1) {
        for (int c = 0; c < p.C; c++) col[c] = (a[c] / 2.0f + 0.5f) * shade * 2.0f - 1.0f;
    } else {
        const float s = p.grey * shade * 2.0f - 1.0f;
        for (int c = 0; c < 3; c++) col[c] = s;
    }
    return true;
}

template <bool IMPLICIT, int MODE>
__global__ __launch_bounds__(256) void sweep_shade_kernel(ShadeParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)p.B * p.V * p.S * p.S) return;
    resolve_pixel(i, p.S, p.ssaa, p.Cout, p.out, p.alpha, [&](int f, int yi, int xi, float col[4]) {
        return shade_sample<IMPLICIT, MODE>(p, f, f / p.V, yi, xi, col);
    });
}

template <bool IMPLICIT>
static void launch_shade(const ShadeParams &p, int mode, hipStream_t st) {
    const int blocks = cdiv((long)p.B * p.V * p.S * p.S, 256);
    if (mode == 0) sweep_shade_kernel<IMPLICIT, 0><<<blocks, 256, 0, st>>>(p);
    else if (mode == 1) sweep_shade_kernel<IMPLICIT, 1><<<blocks, 256, 0, st>>>(p);
    else if (mode == 2) sweep_shade_kernel<IMPLICIT, 2><<<blocks, 256, 0, st>>>(p);
    else sweep_shade_kernel<IMPLICIT, 3><<<blocks, 256, 0, st>>>(p);
}


struct PseudoParams {
    const float *warped;     // [B*V, P] rasterised depth of the posed meshes, unclamped
    const float *rays;       // [P, 3]
    const float *pose;       // [B, V, 12]
    const float *albedo;     // [B, C, P]
    const float *normal;     // [B, P, 3] or NULL
    const float *light;      // [B*V, 4] or NULL
    const float *mask;       // [B, P] or NULL
    float *im;               // [B*V, C, P]
    float *mask_out;         // [B*V, P] or NULL
    int V, S, C, bpf;        // bpf = workgroups per frame
    float lo, hi;
    float k00, k01, k02, k10, k11, k12;
};

__global__ __launch_bounds__(256) void sweep_pseudo_kernel(PseudoParams a) {
    const int f = blockIdx.x / a.bpf;                       // wave-uniform: frame, image, pose and light
    const int p = (blockIdx.x - f * a.bpf) * 256 + threadIdx.x;
    const int S = a.S, P = S * S;
    if (p >= P) return;
    const int b = f / a.V;
    const float *q = a.pose + (size_t)f * 12;
    float d = a.warped[(size_t)f * P + p];
    d = d < a.lo ? a.lo : (d > a.hi ? a.hi : d);
    // q = A^T (d ray - t), the inverse of the posed-vertex map, in double: t = c + t_view - R c has the size of the
    // rotation centre's depth and d ray - t cancels most of it, so in float the texel coordinate would carry several
    // times the rounding of the composed route (which subtracts c first).  A few dozen fp64 operations per pixel of a
    // gather-bound pass.  The normalisation of grid_3d_to_2d and the un-normalisation of grid_sample
    // (align_corners = True) cancel: K q / q.z IS the texel coordinate.
    const double zx = (double)a.rays[3 * p] * d - q[9], zy = (double)a.rays[3 * p + 1] * d - q[10],
                 zz = (double)a.rays[3 * p + 2] * d - q[11];
    const double yx = (zx * q[0] + zy * q[3]) + zz * q[6];
    const double yy = (zx * q[1] + zy * q[4]) + zz * q[7];
    const double yz = (zx * q[2] + zy * q[5]) + zz * q[8];
    const double pa = yx / yz, pb = yy / yz;
    const float ix = (float)((pa * a.k00 + pb * a.k01) + a.k02), iy = (float)((pa * a.k10 + pb * a.k11) + a.k12);
    const float fx = floorf(ix), fy = floorf(iy);
    // a float outside the int range (or NaN) must not hit undefined conversion: such a pixel has no tap in range
    const bool sane = fx >= -2.0f && fx <= (float)S && fy >= -2.0f && fy <= (float)S;
    const int x0 = sane ? (int)fx : -2, y0 = sane ? (int)fy : -2;
    const float wx0 = (fx + 1.0f) - ix, wx1 = ix - fx, wy0 = (fy + 1.0f) - iy, wy1 = iy - fy;
    const float w[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};          // nw, ne, sw, se
    bool in[4];
    int at[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x0 + (k & 1), y = y0 + (k >> 1);
        in[k] = x >= 0 && x < S && y >= 0 && y < S;
        at[k] = in[k] ? y * S + x : 0;                                          // only dereferenced when in range
    }
    float sh[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (a.light) {
        const float *l = a.light + (size_t)f * 4;
        const float la = l[0] / 2.0f + 0.5f, lb = l[1] / 2.0f + 0.5f;
        const float nrm = sqrtf(l[2] * l[2] + l[3] * l[3] + 1.0f);
        const float dx = l[2] / nrm, dy = l[3] / nrm, dz = 1.0f / nrm;
        const float *nb = a.normal + (size_t)b * P * 3;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!in[k]) continue;
            const float *n = nb + (size_t)at[k] * 3;
            const float dot = n[0] * dx + n[1] * dy + n[2] * dz;
            sh[k] = la + lb * (dot > 0.0f ? dot : 0.0f);
        }
    }
    const float *al = a.albedo + (size_t)b * a.C * P;
    float *o = a.im + (size_t)f * a.C * P + p;
    for (int c = 0; c < a.C; c++, al += P, o += P) {
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!in[k]) continue;
            const float t = a.light ? (al[at[k]] / 2.0f + 0.5f) * sh[k] * 2.0f - 1.0f : al[at[k]];
            v += t * w[k];
        }
        *o = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);     // NaN passes through, like torch.clamp
    }
    if (a.mask_out) {
        // mode='nearest': round half to even, zero padding
        const float rx = rintf(ix), ry = rintf(iy);
        const bool inside = rx >= 0.0f && rx <= (float)(S - 1) && ry >= 0.0f && ry <= (float)(S - 1);
        float m = 0.0f;
        if (inside) m = a.mask ? a.mask[(size_t)b * P + (int)ry * S + (int)rx] : 1.0f;
        a.mask_out[(size_t)f * P + p] = m;
    }
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_sweep_verts(const float *verts, const float *pose, float *out, int B, int V, int n_verts,
                               g2s_stream_t stream) {
    G2S_REQUIRE(verts && pose && out, "g2s_sweep_verts: NULL pointer argument");
    G2S_REQUIRE(B > 0 && V > 0 && n_verts > 0, "g2s_sweep_verts: sizes must be positive");
    G2S_REQUIRE(B <= 65535 && V <= 65535 * SWEEP_VPB, "g2s_sweep_verts: B = %d, V = %d exceed the grid", B, V);
    const long row = (long)n_verts * 3;
    const bool wide = row % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid(cdiv(wide ? row / 4 : row, 256), cdiv(V, SWEEP_VPB), B);
    if (wide) sweep_verts_kernel<4><<<grid, 256, 0, as_stream(stream)>>>(verts, pose, out, V, row);
    else sweep_verts_kernel<1><<<grid, 256, 0, as_stream(stream)>>>(verts, pose, out, V, row);
    return check_launch("g2s_sweep_verts");
}

extern "C" int g2s_sweep_shade(const float *verts, const int32_t *faces, const int32_t *face_idx, const float *bary,
                               const float *attr, const float *normal, const float *pose, const float *light, int B,
                               int V, int n_verts, int n_faces, int S, int ssaa, int C, int fill_back, int mode,
                               const float *background, float grey, float *rgb_out, float *alpha_out,
                               g2s_stream_t stream) {
    G2S_REQUIRE(mode >= 0 && mode <= 3, "g2s_sweep_shade: mode %d (0 texture, 1 shaded, 2 shape, 3 normal)", mode);
    G2S_REQUIRE(verts && face_idx && bary && rgb_out && background, "g2s_sweep_shade: NULL pointer argument");
    G2S_REQUIRE(B > 0 && V > 0 && n_verts > 0 && n_faces > 0 && S > 0, "g2s_sweep_shade: sizes must be positive");
    G2S_REQUIRE((long)B * V <= 0x7fffffffL, "g2s_sweep_shade: B * V exceeds int");
    G2S_REQUIRE(ssaa == 1 || ssaa == 2, "g2s_sweep_shade: ssaa must be 1 or 2");
    G2S_REQUIRE(faces || (n_verts == S * S && n_faces == 2 * (S - 1) * (S - 1)),
                "g2s_sweep_shade: implicit topology needs S*S vertices and 2(S-1)^2 faces");
    const bool reads_attr = mode == 0 || mode == 1;
    G2S_REQUIRE(!reads_attr || attr, "g2s_sweep_shade: mode %d reads attr, which is NULL", mode);
    G2S_REQUIRE(!reads_attr || (C >= 1 && C <= 4), "g2s_sweep_shade: C = %d outside 1..4", C);
    G2S_REQUIRE(mode == 0 || (normal && pose), "g2s_sweep_shade: mode %d needs normal and pose", mode);
    G2S_REQUIRE((mode != 1 && mode != 2) || light, "g2s_sweep_shade: mode %d needs light", mode);
    ShadeParams p{};
    p.verts = verts;
    p.faces = faces;
    p.face_idx = face_idx;
    p.bary = bary;
    p.attr = attr;
    p.normal = normal;
    p.pose = pose;
    p.light = light;
    p.out = rgb_out;
    p.alpha = alpha_out;
    p.B = B;
    p.V = V;
    p.N = n_verts;
    p.F = n_faces;
    p.S = S;
    p.is = S * ssaa;
    p.ssaa = ssaa;
    p.C = reads_attr ? C : 3;
    p.Cout = reads_attr ? C : 3;
    p.fill_back = fill_back ? 1 : 0;
    p.grey = grey;
    for (int c = 0; c < p.Cout; c++) p.bg[c] = background[c];
    if (faces) launch_shade<false>(p, mode, as_stream(stream));
    else launch_shade<true>(p, mode, as_stream(stream));
    return check_launch("g2s_sweep_shade");
}

extern "C" int g2s_sweep_pseudo(const float *warped, const float *rays, const float *pose, const float *K,
                                const float *albedo, const float *normal, const float *light, const float *mask,
                                float depth_lo, float depth_hi, int B, int V, int S, int C, float *im_out,
                                float *mask_out, g2s_stream_t stream) {
    G2S_REQUIRE(warped && rays && pose && K && albedo && im_out, "g2s_sweep_pseudo: NULL pointer argument");
    G2S_REQUIRE(B > 0 && V > 0, "g2s_sweep_pseudo: sizes must be positive");
    G2S_REQUIRE(S >= 2 && S <= 16384, "g2s_sweep_pseudo: S = %d outside 2..16384", S);
    G2S_REQUIRE(C >= 1 && C <= 4, "g2s_sweep_pseudo: C = %d outside 1..4", C);
    G2S_REQUIRE((normal == nullptr) == (light == nullptr),
                "g2s_sweep_pseudo: normal and light go together (both, or neither for no relighting)");
    G2S_REQUIRE(depth_lo <= depth_hi, "g2s_sweep_pseudo: depth_lo > depth_hi");
    const long bpf = cdiv((long)S * S, 256);
    // HIP launches at most 2^32 - 1 threads per grid dimension: 256 threads x fewer than 2^24 workgroups
    G2S_REQUIRE((long)B * V * bpf < (1L << 24), "g2s_sweep_pseudo: B * V * ceil(S*S / 256) = %ld workgroups exceed the grid (2^24)",
                (long)B * V * bpf);
    PseudoParams a{};
    a.warped = warped;
    a.rays = rays;
    a.pose = pose;
    a.albedo = albedo;
    a.normal = normal;
    a.light = light;
    a.mask = mask;
    a.im = im_out;
    a.mask_out = mask_out;
    a.V = V;
    a.S = S;
    a.C = C;
    a.bpf = (int)bpf;
    a.lo = depth_lo;
    a.hi = depth_hi;
    a.k00 = K[0]; a.k01 = K[1]; a.k02 = K[2];
    a.k10 = K[3]; a.k11 = K[4]; a.k12 = K[5];
    sweep_pseudo_kernel<<<(unsigned)((long)B * V * bpf), 256, 0, as_stream(stream)>>>(a);
    return check_launch("g2s_sweep_pseudo");
}
