// raster_rgb.hip — texture path of the rasterizer: nr.Renderer.render_rgb as GAN2Shape's
// visualisation helpers use it (GAN2Shape/renderer/renderer.py:196,230,248,272,275: render_yaw,
// render_view, render_given_view(grid_sample=False) with texture cubes from
// renderer/utils.py:83-109), and its backward: the gradient of the texture lookup w.r.t. the textures
// (exact: the forward is affine in them) and w.r.t. the vertices with the winner of every sample held
// fixed (no silhouette term; the external package's edge-sweep heuristic is not rebuilt).
//
// Second pass over the maps the depth rasterizer (raster.hip) saves — winning face id and clamped,
// renormalised barycentric weights per supersample: per sample the texture cube of the winning
// face is read trilinearly at perspective-corrected coordinates
//     t_k = clamp(w_k * (ts - 1) * D / z_k, 0, ts - 1 - eps),   D = 1 / sum_k (w_k / z_k)
// (the reversed fill_back copy of a face reads the cube with axes 0 and 2 swapped), background
// samples take the background colour, then the same vertical flip + 2x2 average as the depth map.
// Semantics follow the external neural_renderer package as recalled in SURVEY.md Appendix A
// (PARITY UNPINNED, like the depth path); the oracle restates them independently on the CPU.
//
// g2s_raster_rgba_fwd / g2s_raster_rgba_bwd are the superset nr.Renderer.render needs: a per-face light factor
// (face_light.hip, indexed by the winner id) multiplies the sample's colour before background selection, and
// alpha is the share of a pixel's samples that have a winner.  The unlit entry points call the same launchers
// with light = alpha_out = grad_light = NULL and run the same template instances as before.
//
// What this file shares is stated elsewhere, once: the winner decode in raster_core.h (winner_verts); the
// perspective weights, the cube coordinates with their clamp state (CubeCoord: forward and the three gradient
// sections read the same cells with the same weights) and the pixel resolve in shade_core.h; the accumulator
// prologue, the merge, the vertex table and the unfix / projection kernels in raster_scatter.h.
#include "g2s_common.h"
#include "raster_core.h"
#include "raster_scatter.h"
#include "shade_core.h"

namespace g2s {

struct RgbParams {
    const float *verts;      // [B, N, 3] camera space (z is what the weights are corrected with)
    const int32_t *faces;    // [F, 3] or NULL (implicit regular grid)
    const int32_t *face_idx; // [B, is, is]
    const float *bary;       // [B, is, is, 3]
    const float *tex;        // [B, F, ts, ts, ts, C]
    float *out;              // [B, C, S, S]
    int B, N, F, S, is, ssaa, ts, C;
    float eps;
    float bg[4];
    const float *light;      // [B, Ftot, 3] or NULL (EXTRA instances only; C == 3)
    float *alpha;            // [B, S, S] or NULL (EXTRA instances only)
    int Ftot;                // F * (1 + fill_back)
};

// EXTRA: the instances of g2s_raster_rgba_fwd (light and / or alpha).  Returns whether the sample has a winner.
template <bool IMPLICIT, bool EXTRA>
__device__ __forceinline__ bool sample_colour(const RgbParams &p, int b, int yi, int xi, float col[4]) {
    const size_t si = ((size_t)b * p.is + yi) * p.is + xi;
    const int fn = p.face_idx[si];
    if (fn < 0) {
        for (int c = 0; c < p.C; c++) col[c] = p.bg[c];
        return false;
    }
    int g, v[3];
    bool rev;
    winner_verts(fn, p.F, p.S, IMPLICIT ? nullptr : p.faces, true, g, rev, v);
    float w[3], z[3], a[3];
    for (int k = 0; k < 3; k++) {
        w[k] = p.bary[3 * si + k];
        z[k] = p.verts[((size_t)b * p.N + v[k]) * 3 + 2];
    }
    const float depth = persp_weights(w, z, a);
    const int ts = p.ts;
    cube_coord(w, z, depth, ts, p.eps).read(p.tex + ((size_t)b * p.F + g) * ts * ts * ts * p.C, rev, ts, p.C, col);
    if (EXTRA && p.light) {
        const float *l = p.light + ((size_t)b * p.Ftot + min(fn, p.Ftot - 1)) * 3;
        for (int c = 0; c < 3; c++) col[c] *= l[c];
    }
    return true;
}

template <bool IMPLICIT, bool EXTRA>
__global__ void raster_rgb_kernel(RgbParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)p.B * p.S * p.S) return;
    resolve_pixel(i, p.S, p.ssaa, p.C, p.out, EXTRA ? p.alpha : nullptr, [&](int b, int yi, int xi, float col[4]) {
        return sample_colour<IMPLICIT, EXTRA>(p, b, yi, xi, col);
    });
}

// Alpha alone (nr.Renderer.render_silhouettes): the resolve with no colour channels, no texture is read.
__global__ void raster_alpha_kernel(const int32_t *face_idx, float *alpha, int B, int S, int ssaa) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * S * S) return;
    const int is = S * ssaa;
    resolve_pixel(i, S, ssaa, 0, nullptr, alpha,
                  [&](int b, int yi, int xi, float *) { return face_idx[((size_t)b * is + yi) * is + xi] >= 0; });
}

// ---------------------------------------------------------------------------------- backward
struct RgbBwdParams {
    const float *verts;      // [B, N, 3]
    const int32_t *faces;    // [F, 3] or NULL (implicit regular grid)
    const int32_t *face_idx; // [B, is, is]
    const float *bary;       // [B, is, is, 3]
    const float *tex;        // [B, F, ts, ts, ts, C]
    const float *grad_rgb;   // [B, C, S, S]
    int B, N, F, S, is, ssaa, ts, C;
    float eps;
    Cam cam;
    void *gtex;  // [B, F, ts, ts, ts, C] sums: float, or 2^-40 fixed point in deterministic mode
    void *gver;  // [B, N, 3] sums of (g_u, g_v, g_z) of the projected vertices, same two forms
    const float *light;  // [B, Ftot, 3] (LIT instances only; C == 3)
    void *glight;        // [B, Ftot, 3] sums, same two forms, or NULL (LIT instances only)
    int Ftot;            // F * (1 + fill_back)
};

// One wave per 8x8-sample tile (4 tiles per workgroup), lane = raster sample, as raster_bwd_samples.
//   textures  adjoint of the trilinear read: the eight corner weights times the sample's share of
//             grad_rgb.  MERGE (ts == 2): every sample of a face reads the same eight cells, so the 8 x C
//             partials of same-face neighbours are merged through shuffles before the atomics;
//             otherwise each sample adds to its own cells.
//   vertices  colour -> t_k (derivative of the trilinear read, zero where a clamp is active)
//             -> a_k = w_k / z_k through t_k = (ts - 1) a_k / sum_j a_j -> (w, z); w are the screen-space
//             barycentrics, whose motion with the projected vertices is dw_k = -(is / 2) w_l (fi[3k] dx_l +
//             fi[3k+1] dy_l) (derivative of the inverse vertex matrix of face_inverse); the lookup position
//             comes from the saved weights, so that forward and backward agree on cell and clamp state.
//             Nine partials per sample, merged and scattered like the depth backward's.
//   light     (LIT: the forward multiplied the sample's colour by light[b, winner]) the incoming colour gradient
//             is scaled by the light for the two gradients above; the light's own gradient is the sum over the
//             winner's samples of grad_colour * unlit colour, three partials per sample that same-face
//             neighbours merge like the others before the atomics.
template <typename ACC, bool WANT_T, bool WANT_V, bool MERGE, bool LIT>
__global__ __launch_bounds__(256) void raster_rgb_bwd_samples(RgbBwdParams p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles_side = (p.is + TILE - 1) / TILE;
    const int tile = blockIdx.x * 4 + wave, b = blockIdx.y;
    if (tile >= tiles_side * tiles_side) return;  // whole wave
    const int xi = (tile % tiles_side) * TILE + (lane & 7), yi = (tile / tiles_side) * TILE + (lane >> 3);
    const bool inside = xi < p.is && yi < p.is;
    const size_t si = ((size_t)b * p.is + (inside ? yi : 0)) * p.is + (inside ? xi : 0);
    int fn = inside ? p.face_idx[si] : -1;
    const int ts = p.ts;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (fn >= 0) {
        const int fr = p.is - 1 - yi;
        const float inv = 1.0f / (float)(p.ssaa * p.ssaa);
        bool any = false;
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < p.C) {
                g[c] = p.grad_rgb[(((size_t)b * p.C + c) * p.S + fr / p.ssaa) * p.S + xi / p.ssaa] * inv;
                any = any || g[c] != 0.0f;
            }
        if (!any) fn = -1;  // masked pixels contribute exact zeros
    }
    int v[3] = {0, 0, 0};
    float w[3] = {0, 0, 0}, z[3] = {1, 1, 1}, a[3] = {0, 0, 0};
    float depth = 0.0f;
    CubeCoord cc{};   // the forward's lookup position, from the same saved weights: same cell, same clamp state
    bool rev = false;
    int gidx = 0;
    if (fn >= 0) {
        winner_verts(fn, p.F, p.S, p.faces, true, gidx, rev, v);
        for (int k = 0; k < 3; k++) {
            w[k] = p.bary[3 * si + k];
            z[k] = p.verts[((size_t)b * p.N + v[k]) * 3 + 2];
        }
        depth = persp_weights(w, z, a);
        cc = cube_coord(w, z, depth, ts, p.eps);
    }
    const size_t cube = ((size_t)b * p.F + gidx) * ts * ts * ts * p.C;

    if (LIT) {
        float lp[3] = {0.0f, 0.0f, 0.0f};
        if (fn >= 0) {
            if (p.glight) {  // grad_colour * unlit colour: the forward's trilinear read again
                cc.read(p.tex + cube, rev, ts, 3, lp);
                for (int c = 0; c < 3; c++) lp[c] *= g[c];
            }
            const float *l = p.light + ((size_t)b * p.Ftot + min(fn, p.Ftot - 1)) * 3;
            for (int c = 0; c < 3; c++) g[c] *= l[c];
        }
        if (p.glight) {  // uniform: every lane takes part in the shuffles
            int fl = fn;
            merge_same_face(lp, fl, lane);
            if (fl >= 0 && fl < p.Ftot) {
                ACC *dst = reinterpret_cast<ACC *>(p.glight) + ((size_t)b * p.Ftot + fl) * 3;
                for (int c = 0; c < 3; c++) acc_add(dst + c, lp[c]);
            }
        }
    }

    if (WANT_T) {
        ACC *const gt = reinterpret_cast<ACC *>(p.gtex);
        if (MERGE) {
            float part[32];
#pragma unroll
            for (int pn = 0; pn < 8; pn++) {
                const float wt = cc.weight(pn);
#pragma unroll
                for (int c = 0; c < 4; c++) part[4 * pn + c] = fn >= 0 ? wt * g[c] : 0.0f;
            }
            int ft = fn;
            merge_same_face(part, ft, lane);
            if (ft >= 0) {
#pragma unroll
                for (int pn = 0; pn < 8; pn++) {
                    ACC *dst = gt + cube + (size_t)cc.cell(pn, rev, ts) * p.C;
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if (c < p.C) acc_add(dst + c, part[4 * pn + c]);
                }
            }
        } else if (fn >= 0) {
            for (int pn = 0; pn < 8; pn++) {
                const float wt = cc.weight(pn);
                if (wt == 0.0f) continue;
                ACC *dst = gt + cube + (size_t)cc.cell(pn, rev, ts) * p.C;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (c < p.C) acc_add(dst + c, wt * g[c]);
            }
        }
    }

    if (WANT_V) {
        ACC *const gout_b = reinterpret_cast<ACC *>(p.gver) + (size_t)b * p.N * 3;
        int fv = fn;
        float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (fv >= 0 && !(cc.live[0] || cc.live[1] || cc.live[2])) fv = -1;  // constant under every clamp: exact zeros
        if (fv >= 0) {
            // d colour . g / d t_k: the corner sums with the k-th factor replaced by its derivative (-1, +1)
            float gtk[3] = {0.0f, 0.0f, 0.0f};
            for (int pn = 0; pn < 8; pn++) {
                const float *tx = p.tex + cube + (size_t)cc.cell(pn, rev, ts) * p.C;
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (c < p.C) s += g[c] * tx[c];
                const float f[3] = {cc.factor(pn, 0), cc.factor(pn, 1), cc.factor(pn, 2)};
                gtk[0] += (((pn >> 0) & 1) ? s : -s) * (f[1] * f[2]);
                gtk[1] += (((pn >> 1) & 1) ? s : -s) * (f[0] * f[2]);
                gtk[2] += (((pn >> 2) & 1) ? s : -s) * (f[0] * f[1]);
            }
            for (int k = 0; k < 3; k++)
                if (!cc.live[k]) gtk[k] = 0.0f;
            // t_k = (ts - 1) a_k D, D = 1 / sum_j a_j:  g_a[j] = (ts - 1) D (g_t[j] - D sum_k g_t[k] a_k)
            const float dot = (gtk[0] * a[0] + gtk[1] * a[1] + gtk[2] * a[2]) * depth;
            float gw[3], gz[3];
            for (int k = 0; k < 3; k++) {
                const float ga = (float)(ts - 1) * depth * (gtk[k] - dot);
                gw[k] = ga / z[k];
                gz[k] = -ga * a[k] / z[k];
            }
            float px[3], py[3], fi[9];
            for (int k = 0; k < 3; k++) {
                const float *q = p.verts + ((size_t)b * p.N + v[k]) * 3;
                project(q[0], q[1], q[2], p.cam, px[k], py[k]);
            }
            face_inverse(px[0], py[0], px[1], py[1], px[2], py[2], p.is, fi);
            const float sx = -(gw[0] * fi[0] + gw[1] * fi[3] + gw[2] * fi[6]) * (float)p.is / 2.0f;
            const float sy = -(gw[0] * fi[1] + gw[1] * fi[4] + gw[2] * fi[7]) * (float)p.is / 2.0f;
            for (int k = 0; k < 3; k++) {
                acc[3 * k] = sx * w[k];
                acc[3 * k + 1] = sy * w[k];
                acc[3 * k + 2] = gz[k];
            }
        }
        merge_same_face(acc, fv, lane);
        __shared__ VertexTable<ACC> table[4];
        vt_clear(table[wave], lane);
        if (fv >= 0)
            for (int k = 0; k < 3; k++) vt_add(table[wave], v[k], acc[3 * k], acc[3 * k + 1], acc[3 * k + 2], gout_b);
        vt_flush(table[wave], lane, gout_b);
    }
}

template <typename ACC, bool MERGE, bool LIT>
static void launch_rgb_bwd_lit(const RgbBwdParams &p, bool want_t, bool want_v, hipStream_t st) {
    const int tiles = cdiv(p.is, TILE) * cdiv(p.is, TILE);
    const dim3 grid(cdiv(tiles, 4), p.B);
    if (want_t && want_v) raster_rgb_bwd_samples<ACC, true, true, MERGE, LIT><<<grid, 256, 0, st>>>(p);
    else if (want_t) raster_rgb_bwd_samples<ACC, true, false, MERGE, LIT><<<grid, 256, 0, st>>>(p);
    else raster_rgb_bwd_samples<ACC, false, true, false, LIT><<<grid, 256, 0, st>>>(p);
}

template <typename ACC, bool MERGE>
static void launch_rgb_bwd(const RgbBwdParams &p, bool want_t, bool want_v, hipStream_t st) {
    if (p.light) launch_rgb_bwd_lit<ACC, MERGE, true>(p, want_t, want_v, st);
    else launch_rgb_bwd_lit<ACC, MERGE, false>(p, want_t, want_v, st);
}

}  // namespace g2s

using namespace g2s;

// The one host launcher of the forward kernel; `who` names the entry point in a launch error.
static int rgb_fwd(const char *who, const float *verts, const int32_t *faces, const int32_t *face_idx,
                   const float *bary, const float *textures, const float *light, int B, int n_verts, int n_faces,
                   int S, int ssaa, int ts, int C, int fill_back, const float *background, float eps, float *rgb_out,
                   float *alpha_out, g2s_stream_t stream) {
    G2S_REQUIRE(verts && face_idx && bary && textures && rgb_out && background, "NULL pointer argument");
    G2S_REQUIRE(B > 0 && n_verts > 0 && n_faces > 0 && S > 0, "sizes must be positive");
    G2S_REQUIRE(ssaa == 1 || ssaa == 2, "ssaa must be 1 or 2");
    G2S_REQUIRE(ts >= 1 && ts <= 8 && C >= 1 && C <= 4, "texture size 1..8, 1..4 channels");
    G2S_REQUIRE(faces || (n_verts == S * S && n_faces == 2 * (S - 1) * (S - 1)),
                "implicit topology needs S*S vertices and 2(S-1)^2 faces");
    G2S_REQUIRE(!light || C == 3, "a light factor needs 3 channels");
    RgbParams p{};
    p.light = light;
    p.alpha = alpha_out;
    p.Ftot = n_faces * (fill_back ? 2 : 1);
    p.verts = verts;
    p.faces = faces;
    p.face_idx = face_idx;
    p.bary = bary;
    p.tex = textures;
    p.out = rgb_out;
    p.B = B;
    p.N = n_verts;
    p.F = n_faces;
    p.S = S;
    p.is = S * ssaa;
    p.ssaa = ssaa;
    p.ts = ts;
    p.C = C;
    p.eps = eps;
    for (int c = 0; c < C; c++) p.bg[c] = background[c];
    const long n = (long)B * S * S;
    const bool extra = light || alpha_out;
    if (faces && extra) raster_rgb_kernel<false, true><<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(p);
    else if (faces) raster_rgb_kernel<false, false><<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(p);
    else if (extra) raster_rgb_kernel<true, true><<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(p);
    else raster_rgb_kernel<true, false><<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(p);
    return check_launch(who);
}

extern "C" int g2s_raster_rgb_fwd(const float *verts, const int32_t *faces, const int32_t *face_idx,
                                  const float *bary, const float *textures, int B, int n_verts, int n_faces,
                                  int S, int ssaa, int ts, int C, const float *background, float eps,
                                  float *rgb_out, g2s_stream_t stream) {
    return rgb_fwd("g2s_raster_rgb_fwd", verts, faces, face_idx, bary, textures, nullptr, B, n_verts, n_faces, S, ssaa,
                   ts, C, 0, background, eps, rgb_out, nullptr, stream);
}

extern "C" int g2s_raster_rgba_fwd(const float *verts, const int32_t *faces, const int32_t *face_idx,
                                   const float *bary, const float *textures, const float *light, int B, int n_verts,
                                   int n_faces, int S, int ssaa, int ts, int C, int fill_back,
                                   const float *background, float eps, float *rgb_out, float *alpha_out,
                                   g2s_stream_t stream) {
    if (!textures && !rgb_out && !light) {  // alpha alone: no texture pass
        G2S_REQUIRE(face_idx && alpha_out, "NULL pointer argument");
        G2S_REQUIRE(B > 0 && S > 0, "sizes must be positive");
        G2S_REQUIRE(ssaa == 1 || ssaa == 2, "ssaa must be 1 or 2");
        raster_alpha_kernel<<<cdiv((long)B * S * S, 256), 256, 0, as_stream(stream)>>>(face_idx, alpha_out, B, S, ssaa);
        return check_launch("g2s_raster_rgba_fwd");
    }
    return rgb_fwd("g2s_raster_rgba_fwd", verts, faces, face_idx, bary, textures, light, B, n_verts, n_faces, S, ssaa,
                   ts, C, fill_back, background, eps, rgb_out, alpha_out, stream);
}

static size_t rgb_bwd_tex_elems(int B, int n_faces, int ts, int C) { return (size_t)B * n_faces * ts * ts * ts * C; }

extern "C" size_t g2s_raster_rgb_bwd_workspace_bytes(int B, int n_verts, int n_faces, int ts, int C) {
    if (B <= 0 || n_verts <= 0 || n_faces <= 0 || ts <= 0 || C <= 0) return 0;
    return (rgb_bwd_tex_elems(B, n_faces, ts, C) + (size_t)B * n_verts * 3) * sizeof(long long) + 256;
}

extern "C" size_t g2s_raster_rgba_bwd_workspace_bytes(int B, int n_verts, int n_faces, int ts, int C, int fill_back) {
    const size_t unlit = g2s_raster_rgb_bwd_workspace_bytes(B, n_verts, n_faces, ts, C);
    return unlit ? unlit + (size_t)B * n_faces * (fill_back ? 2 : 1) * 3 * sizeof(long long) : 0;
}

// The one host launcher of the backward kernels; `who` names the entry point in its messages.
static int rgb_bwd(const char *who, const float *verts, const int32_t *faces, const int32_t *face_idx,
                   const float *bary, const float *textures, const float *light, const float *grad_rgb, int B,
                   int n_verts, int n_faces, int S, const float *K, float orig_size, int ssaa, int ts, int C,
                   int fill_back, float eps, float *grad_textures, float *grad_verts, float *grad_light,
                   void *workspace, size_t workspace_bytes, int acc_is_zero, g2s_stream_t stream) {
    G2S_REQUIRE(verts && face_idx && bary && textures && grad_rgb, "NULL pointer argument");
    G2S_REQUIRE(!light || C == 3, "a light factor needs 3 channels");
    G2S_REQUIRE(light || !grad_light, "grad_light needs light");
    G2S_REQUIRE(grad_textures || grad_verts, "grad_textures and grad_verts are both NULL: nothing to compute");
    G2S_REQUIRE(B > 0 && n_verts > 0 && n_faces > 0 && S > 0, "sizes must be positive");
    G2S_REQUIRE(ssaa == 1 || ssaa == 2, "ssaa must be 1 or 2");
    G2S_REQUIRE(ts >= 1 && ts <= 8 && C >= 1 && C <= 4, "texture size 1..8, 1..4 channels");
    G2S_REQUIRE(faces || (n_verts == S * S && n_faces == 2 * (S - 1) * (S - 1)),
                "implicit topology needs S*S vertices and 2(S-1)^2 faces");
    RgbBwdParams p{};
    int rc = make_cam(K, orig_size, p.cam);
    if (rc) return rc;
    p.verts = verts;
    p.faces = faces;
    p.face_idx = face_idx;
    p.bary = bary;
    p.tex = textures;
    p.grad_rgb = grad_rgb;
    p.B = B;
    p.N = n_verts;
    p.F = n_faces;
    p.S = S;
    p.is = S * ssaa;
    p.ssaa = ssaa;
    p.ts = ts;
    p.C = C;
    p.eps = eps;
    p.light = light;
    p.Ftot = n_faces * (fill_back ? 2 : 1);
    hipStream_t st = as_stream(stream);
    const size_t nt = rgb_bwd_tex_elems(B, n_faces, ts, C), nv = (size_t)B * n_verts * 3;
    const size_t nl = grad_light ? (size_t)B * p.Ftot * 3 : 0;
    const bool want_t = grad_textures != nullptr, want_v = grad_verts != nullptr;
    // in the fixed-point workspace: textures, then vertices, then light
    const ScatterTarget targets[3] = {{grad_light, nl, "grad_light"}, {grad_textures, nt, "grad_textures"},
                                      {grad_verts, nv, "grad_verts"}};
    const size_t need = g2s_raster_rgb_bwd_workspace_bytes(B, n_verts, n_faces, ts, C) + nl * sizeof(long long);
    long long *fix;
    rc = scatter_begin(who, need, workspace, workspace_bytes, acc_is_zero, st, targets, 3, fix);
    if (rc) return rc;
    if (fix) {
        p.gtex = fix;
        p.gver = fix + nt;
        p.glight = grad_light ? fix + nt + nv : nullptr;
        if (ts == 2) launch_rgb_bwd<long long, true>(p, want_t, want_v, st);
        else launch_rgb_bwd<long long, false>(p, want_t, want_v, st);
        if (want_t) scatter_unfix<false><<<cdiv((long)nt, 256), 256, 0, st>>>(fix, grad_textures, (long)nt);
        if (grad_light) scatter_unfix<false><<<cdiv((long)nl, 256), 256, 0, st>>>(fix + nt + nv, grad_light, (long)nl);
    } else {
        p.gtex = grad_textures;
        p.gver = grad_verts;
        p.glight = grad_light;
        if (ts == 2) launch_rgb_bwd<float, true>(p, want_t, want_v, st);
        else launch_rgb_bwd<float, false>(p, want_t, want_v, st);
    }
    if (want_v)
        scatter_project<<<cdiv((long)B * n_verts, 256), 256, 0, st>>>(verts, grad_verts, fix ? fix + nt : nullptr, p.cam,
                                                                      (long)B * n_verts);
    return check_launch(who);
}

extern "C" int g2s_raster_rgb_bwd(const float *verts, const int32_t *faces, const int32_t *face_idx,
                                  const float *bary, const float *textures, const float *grad_rgb, int B,
                                  int n_verts, int n_faces, int S, const float *K, float orig_size, int ssaa,
                                  int ts, int C, float eps, float *grad_textures, float *grad_verts,
                                  void *workspace, size_t workspace_bytes, int acc_is_zero, g2s_stream_t stream) {
    return rgb_bwd("g2s_raster_rgb_bwd", verts, faces, face_idx, bary, textures, nullptr, grad_rgb, B, n_verts, n_faces,
                   S, K, orig_size, ssaa, ts, C, 0, eps, grad_textures, grad_verts, nullptr, workspace, workspace_bytes,
                   acc_is_zero, stream);
}

extern "C" int g2s_raster_rgba_bwd(const float *verts, const int32_t *faces, const int32_t *face_idx,
                                   const float *bary, const float *textures, const float *light,
                                   const float *grad_rgb, int B, int n_verts, int n_faces, int S, const float *K,
                                   float orig_size, int ssaa, int ts, int C, int fill_back, float eps,
                                   float *grad_textures, float *grad_verts, float *grad_light, void *workspace,
                                   size_t workspace_bytes, int acc_is_zero, g2s_stream_t stream) {
    return rgb_bwd("g2s_raster_rgba_bwd", verts, faces, face_idx, bary, textures, light, grad_rgb, B, n_verts, n_faces,
                   S, K, orig_size, ssaa, ts, C, fill_back, eps, grad_textures, grad_verts, grad_light, workspace,
                   workspace_bytes, acc_is_zero, stream);
}
