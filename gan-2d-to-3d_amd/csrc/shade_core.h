// shade_core.h — per-sample arithmetic of the passes that colour the maps the depth rasterizer saves (raster_rgb.hip,
// sweep.hip), and the loop that resolves a pixel from its samples.
//
// Plain inline functions like raster_core.h: usable from HIP device code and from the host harness
// (tests/raster_tile_emulation.cpp), which renders a texture pass with them on the CPU.  Each rule is stated once:
// the perspective correction, the clamp state of the cube coordinates that forward and backward must share, the
// axis swap of the reversed fill_back copy, and the dy-then-dx summation order of the supersamples.  The including
// translation unit is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include "raster_core.h"

namespace g2s {

// Perspective correction of the screen-space weights w by the camera-space depths z of the winner's vertices:
// a_k = w_k / z_k, returns D = 1 / sum_k a_k (the sample's depth).  The corrected weight of vertex k is a_k D.
G2S_HD float persp_weights(const float w[3], const float z[3], float a[3]) {
    for (int k = 0; k < 3; k++) a[k] = w[k] / z[k];
    return 1.0f / (a[0] + a[1] + a[2]);
}

// Where one sample reads its face's texture cube [ts, ts, ts, C]:
//     t_k = clamp(w_k (ts - 1) D / z_k, 0, ts - 1 - eps),   ti = (int)t,   tf = t - ti,
// live[k] = t_k lies strictly between its clamps (under a clamp the read does not move with the vertices).
// Corner pn in 0..7 takes the upper cell along axis k when bit k of pn is set.
struct CubeCoord {
    int ti[3];
    float tf[3];
    bool live[3];

    G2S_HD float factor(int pn, int k) const { return ((pn >> k) & 1) ? tf[k] : 1.0f - tf[k]; }

    // trilinear weight of corner pn
    G2S_HD float weight(int pn) const {
        float wt = 1.0f;
        for (int k = 0; k < 3; k++) wt *= factor(pn, k);
        return wt;
    }

    // cell of corner pn in the geometric face's cube; the reversed copy's cube is
    // textures.permute(0, 1, 4, 3, 2, 5): axes 0 and 2 swapped
    G2S_HD int cell(int pn, bool rev, int ts) const {
        int idx[3];
        for (int k = 0; k < 3; k++)
            idx[k] = ((pn >> k) & 1) ? (ti[k] + 1 < ts - 1 ? ti[k] + 1 : ts - 1) : ti[k];   // weight 0 there when ts == 1
        return rev ? (idx[2] * ts + idx[1]) * ts + idx[0] : (idx[0] * ts + idx[1]) * ts + idx[2];
    }

    // col[c] = the trilinear read of channel c < C of `cube`
    G2S_HD void read(const float *cube, bool rev, int ts, int C, float *col) const {
        for (int c = 0; c < C; c++) col[c] = 0.0f;
        for (int pn = 0; pn < 8; pn++) {
            const float wt = weight(pn);
            const float *tx = cube + (size_t)cell(pn, rev, ts) * C;
            for (int c = 0; c < C; c++) col[c] += wt * tx[c];
        }
    }
};

G2S_HD CubeCoord cube_coord(const float w[3], const float z[3], float depth, int ts, float eps) {
    CubeCoord cc;
    const float hi = (float)(ts - 1) - eps;
    for (int k = 0; k < 3; k++) {
        const float tu = w[k] * (float)(ts - 1) * (depth / z[k]);
        cc.live[k] = tu > 0.0f && tu < hi;
        float t = fmaxf(tu, 0.0f);
        t = fminf(t, hi);
        cc.ti[k] = (int)t;
        cc.tf[k] = t - (float)cc.ti[k];
    }
    return cc;
}

// Output pixel i of [n, S, S] from its ssaa x ssaa raster samples: vertical flip (pixel row r reads the raster rows
// is - 1 - (r ssaa + dy)), colours summed from zero with dy outer and dx inner, then
//     out[n, C, S, S] = sum / ssaa^2,   alpha[n, S, S] = samples with a winner / ssaa^2   (alpha may be NULL).
// sample(f, yi, xi, col) fills col[0..C) for raster sample (yi, xi) of image f and returns whether it has a winner.
template <typename SAMPLE>
G2S_HD void resolve_pixel(long i, int S, int ssaa, int C, float *out, float *alpha, SAMPLE sample) {
    const int f = (int)(i / ((long)S * S));
    const int r = (int)((i / S) % S), c0 = (int)(i % S), is = S * ssaa;
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int covered = 0;
    for (int dy = 0; dy < ssaa; dy++)
        for (int dx = 0; dx < ssaa; dx++) {
            float col[4];
            if (sample(f, is - 1 - (r * ssaa + dy), c0 * ssaa + dx, col)) covered++;
            for (int c = 0; c < C; c++) sum[c] += col[c];
        }
    const float inv = 1.0f / (float)(ssaa * ssaa);
    for (int c = 0; c < C; c++) out[(((size_t)f * C + c) * S + r) * S + c0] = sum[c] * inv;
    if (alpha) alpha[((size_t)f * S + r) * S + c0] = (float)covered * inv;
}

}  // namespace g2s
