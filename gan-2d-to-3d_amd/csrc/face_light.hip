// face_light.hip — per-face light factor of the textured renderer: nr.lighting as nr.Renderer.render /
// render_rgb apply it (ambient + directional, flat shading per face), and its backward w.r.t. the vertices.
//
// Evaluated on camera-space vertices (after R, t, BEFORE projection).  For the face (v0, v1, v2):
//     n        = cross(v0 - v1, v2 - v1) / max(|cross|, 1e-5)
//     light[c] = ambient[c] + directional[c] * max(0, dot(n, direction))         c = 0..2
// with ambient = intensity_ambient * color_ambient and directional = intensity_directional * color_directional
// folded on the host.  The reversed fill_back copy of a face has vertex order (v2, v1, v0), hence the normal -n
// and the term max(0, -dot(n, direction)).  The output is indexed like the winner ids the depth rasterizer
// stores in face_idx (reversed copies at f + n_faces), so the texture pass (raster_rgb.hip) reads it with the
// id it already holds.  Semantics follow the external neural_renderer package as recalled in SURVEY.md
// Appendix A (PARITY UNPINNED, like the rasterizer); the tests restate them in float64.
//
// One thread per geometric face handles both orientations: the normal is computed once.  Compiled with
// -ffp-contract=off so that forward and backward evaluate dot(n, direction) with the same roundings and agree
// on which side of the max(0, .) a face lies.
#include <climits>
#include "g2s_common.h"
#include "raster_core.h"
#include "raster_scatter.h"

namespace g2s {

struct LightParams {
    const float *verts;    // [B, N, 3] camera space
    const int32_t *faces;  // [F, 3] or NULL (implicit regular grid)
    int B, N, F, S, fill_back;
    float amb[3], dirc[3], dir[3];
    float *light;             // fwd: [B, F * (1 + fill_back), 3]
    const float *grad_light;  // bwd: same layout
    void *gver;               // bwd: [B, N, 3] sums: float (grad_verts itself), or 2^-40 fixed point
};

// Vertex ids and the un-normalised normal of face g of image b; false when an id is out of range.
__device__ __forceinline__ bool face_cross(const LightParams &p, int b, int g, int v[3], float a[3], float e[3],
                                           float c[3]) {
    bool rev;
    winner_verts(g, p.F, p.S, p.faces, false, g, rev, v);   // g < F: the face itself, never its reversed copy
    for (int k = 0; k < 3; k++)
        if ((unsigned)v[k] >= (unsigned)p.N) return false;
    const float *q0 = p.verts + ((size_t)b * p.N + v[0]) * 3;
    const float *q1 = p.verts + ((size_t)b * p.N + v[1]) * 3;
    const float *q2 = p.verts + ((size_t)b * p.N + v[2]) * 3;
    for (int k = 0; k < 3; k++) {
        a[k] = q0[k] - q1[k];
        e[k] = q2[k] - q1[k];
    }
    c[0] = a[1] * e[2] - a[2] * e[1];
    c[1] = a[2] * e[0] - a[0] * e[2];
    c[2] = a[0] * e[1] - a[1] * e[0];
    return true;
}

__global__ __launch_bounds__(256) void face_light_fwd_kernel(LightParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)p.B * p.F) return;
    const int b = (int)(i / p.F), g = (int)(i % p.F);
    int v[3];
    float a[3], e[3], c[3];
    float d = 0.0f;
    if (face_cross(p, b, g, v, a, e, c)) {
        const float len = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const float inv = 1.0f / fmaxf(len, 1e-5f);
        d = (c[0] * inv) * p.dir[0] + (c[1] * inv) * p.dir[1] + (c[2] * inv) * p.dir[2];
    }
    const int ftot = p.F * (1 + p.fill_back);
    float *front = p.light + ((size_t)b * ftot + g) * 3;
    const float df = fmaxf(d, 0.0f), dr = fmaxf(-d, 0.0f);
    for (int k = 0; k < 3; k++) front[k] = p.amb[k] + p.dirc[k] * df;
    if (p.fill_back) {
        float *back = front + (size_t)p.F * 3;
        for (int k = 0; k < 3; k++) back[k] = p.amb[k] + p.dirc[k] * dr;
    }
}

// d light / d verts: through the max (the side that is on), the dot product, the normalisation (no gradient
// while its 1e-5 clamp is active) and the cross product; nine adds per face whose gradient is not zero.
template <typename ACC>
__global__ __launch_bounds__(256) void face_light_bwd_kernel(LightParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)p.B * p.F) return;
    const int b = (int)(i / p.F), g = (int)(i % p.F);
    int v[3];
    float a[3], e[3], c[3];
    if (!face_cross(p, b, g, v, a, e, c)) return;
    const float len = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (!(len > 1e-5f)) return;
    const float inv = 1.0f / len;
    const float n[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
    const float d = n[0] * p.dir[0] + n[1] * p.dir[1] + n[2] * p.dir[2];
    const int ftot = p.F * (1 + p.fill_back);
    const float *gf = p.grad_light + ((size_t)b * ftot + g) * 3;
    float gd = 0.0f;
    if (d > 0.0f) {
        gd = gf[0] * p.dirc[0] + gf[1] * p.dirc[1] + gf[2] * p.dirc[2];
    } else if (d < 0.0f && p.fill_back) {
        const float *gr = gf + (size_t)p.F * 3;
        gd = -(gr[0] * p.dirc[0] + gr[1] * p.dirc[1] + gr[2] * p.dirc[2]);
    }
    if (gd == 0.0f) return;
    // d = dot(c, dir) / |c|:  g_c = gd / |c| * (dir - n d);  c = a x e:  g_a = e x g_c,  g_e = g_c x a
    float gc[3];
    for (int k = 0; k < 3; k++) gc[k] = gd * inv * (p.dir[k] - n[k] * d);
    const float ga[3] = {e[1] * gc[2] - e[2] * gc[1], e[2] * gc[0] - e[0] * gc[2], e[0] * gc[1] - e[1] * gc[0]};
    const float ge[3] = {gc[1] * a[2] - gc[2] * a[1], gc[2] * a[0] - gc[0] * a[2], gc[0] * a[1] - gc[1] * a[0]};
    ACC *const out = reinterpret_cast<ACC *>(p.gver) + (size_t)b * p.N * 3;
    for (int k = 0; k < 3; k++) {
        acc_add(out + (size_t)v[0] * 3 + k, ga[k]);
        acc_add(out + (size_t)v[1] * 3 + k, -(ga[k] + ge[k]));
        acc_add(out + (size_t)v[2] * 3 + k, ge[k]);
    }
}

static int light_args(LightParams &p, const float *verts, const int32_t *faces, int B, int n_verts, int n_faces, int S,
                      int fill_back, const float *directional, const float *direction) {
    G2S_REQUIRE(verts && directional && direction, "NULL pointer argument");
    G2S_REQUIRE(B > 0 && n_verts > 0 && n_faces > 0, "sizes must be positive");
    G2S_REQUIRE(faces || (S >= 2 && n_verts == S * S && n_faces == 2 * (S - 1) * (S - 1)),
                "implicit topology needs S*S vertices and 2(S-1)^2 faces");
    G2S_REQUIRE((long)n_faces * 2 < INT_MAX, "too many faces");
    p.verts = verts;
    p.faces = faces;
    p.B = B;
    p.N = n_verts;
    p.F = n_faces;
    p.S = S;
    p.fill_back = fill_back ? 1 : 0;
    for (int k = 0; k < 3; k++) {
        p.dirc[k] = directional[k];
        p.dir[k] = direction[k];
    }
    return G2S_OK;
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_face_light_fwd(const float *verts, const int32_t *faces, int B, int n_verts, int n_faces, int S,
                                  int fill_back, const float *ambient, const float *directional,
                                  const float *direction, float *light_out, g2s_stream_t stream) {
    G2S_REQUIRE(ambient && light_out, "NULL pointer argument");
    LightParams p{};
    const int rc = light_args(p, verts, faces, B, n_verts, n_faces, S, fill_back, directional, direction);
    if (rc) return rc;
    for (int k = 0; k < 3; k++) p.amb[k] = ambient[k];
    p.light = light_out;
    face_light_fwd_kernel<<<cdiv((long)B * n_faces, 256), 256, 0, as_stream(stream)>>>(p);
    return check_launch("g2s_face_light_fwd");
}

extern "C" int g2s_face_light_bwd(const float *verts, const int32_t *faces, const float *grad_light, int B,
                                  int n_verts, int n_faces, int S, int fill_back, const float *directional,
                                  const float *direction, float *grad_verts, void *workspace,
                                  size_t workspace_bytes, int acc_is_zero, g2s_stream_t stream) {
    G2S_REQUIRE(grad_light && grad_verts, "NULL pointer argument");
    LightParams p{};
    int rc = light_args(p, verts, faces, B, n_verts, n_faces, S, fill_back, directional, direction);
    if (rc) return rc;
    p.grad_light = grad_light;
    hipStream_t st = as_stream(stream);
    const size_t nv = (size_t)B * n_verts * 3;
    const int blocks = cdiv((long)B * n_faces, 256);
    const ScatterTarget target{grad_verts, nv, "grad_verts"};
    long long *fix;
    rc = scatter_begin("g2s_raster_bwd", g2s_raster_bwd_workspace_bytes(B, n_verts), workspace, workspace_bytes,
                       acc_is_zero, st, &target, 1, fix);
    if (rc) return rc;
    if (fix) {
        p.gver = fix;
        face_light_bwd_kernel<long long><<<blocks, 256, 0, st>>>(p);
        // as in default mode, where the atomics add onto whatever an uncleared grad_verts holds
        if (acc_is_zero) scatter_unfix<true><<<cdiv((long)nv, 256), 256, 0, st>>>(fix, grad_verts, (long)nv);
        else scatter_unfix<false><<<cdiv((long)nv, 256), 256, 0, st>>>(fix, grad_verts, (long)nv);
    } else {
        p.gver = grad_verts;
        face_light_bwd_kernel<float><<<blocks, 256, 0, st>>>(p);
    }
    return check_launch("g2s_face_light_bwd");
}
