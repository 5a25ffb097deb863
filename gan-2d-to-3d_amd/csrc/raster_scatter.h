// raster_scatter.h — gradient scatter shared by the rasterizer's two backward passes (raster.hip:
// depth, raster_rgb.hip: texture lookup).  Both run one wave per 8x8-sample tile, lane = raster
// sample, and end the same way: neighbouring samples of one face merge their partial sums through
// shuffles, the per-vertex partials of a tile meet in a per-wave LDS table keyed by vertex id, each
// distinct vertex reaches memory once, and one thread per vertex maps (g_u, g_v, g_z) of the
// projected vertex back to camera xyz.  Device code only (HIP).
#pragma once
#include "g2s_common.h"
#include "raster_core.h"

namespace g2s {

constexpr int TILE = 8;      // samples per tile side (64 samples = one wavefront)

// Deterministic mode accumulates in 64-bit fixed point (LDS and global integer atomics): the sums no
// longer depend on the order the waves arrive in.  Resolution 2^-40 ~ 9e-13, range +-8.4e6 per
// component; a non-finite contribution is not representable and is dropped.
constexpr float FIX_SCALE = 1099511627776.0f;  // 2^40
__device__ __forceinline__ long long to_fix(float v) { return __float2ll_rn(v * FIX_SCALE); }
__device__ __forceinline__ float from_fix(long long v) { return (float)((double)v * (1.0 / 1099511627776.0)); }
__device__ __forceinline__ void acc_add(float *dst, float v) { unsafeAtomicAdd(dst, v); }
__device__ __forceinline__ void acc_add(long long *dst, float v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)to_fix(v));
}
__device__ __forceinline__ void acc_add(long long *dst, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)v);
}
__device__ __forceinline__ void lds_add(float *dst, float v) { atomicAdd(dst, v); }
__device__ __forceinline__ void lds_add(long long *dst, float v) { acc_add(dst, v); }

// The 2x2 super-samples of a pixel mostly hit the same face: x- and then y-neighbours of the tile
// with the same winning face `fn` merge their N partial sums, and the upper lane of a merged pair
// retires (fn = -1), so a face receives one set of atomics per merged group instead of one per sample.
template <int N>
__device__ __forceinline__ void merge_same_face(float (&acc)[N], int &fn, int lane) {
#pragma unroll
    for (int step = 0; step < 2; step++) {
        const int m = step ? 8 : 1;
        const int pfn = __shfl_xor(fn, m);
        const bool same = fn >= 0 && pfn == fn;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const float o = __shfl_xor(acc[k], m);
            if (same) acc[k] += o;
        }
        if (same && (lane & m)) fn = -1;  // the upper lane of a merged pair retires
    }
}

// Per-wave LDS hash table keyed by vertex id: neighbouring faces of a tile share vertices, so the
// tile's contributions are summed with LDS atomics and each distinct vertex reaches global memory
// once (three atomics) instead of once per merged sample group and corner.
constexpr int VT_SLOTS = 128;
template <typename ACC>
struct VertexTable {
    int key[VT_SLOTS];
    ACC val[VT_SLOTS][3];
};

template <typename ACC>
__device__ __forceinline__ void vt_clear(VertexTable<ACC> &t, int lane) {
    for (int i = lane; i < VT_SLOTS; i += 64) {
        t.key[i] = -1;
        t.val[i][0] = t.val[i][1] = t.val[i][2] = (ACC)0;
    }
    __builtin_amdgcn_wave_barrier();
}

// gout: this image's [N, 3] accumulation rows.
template <typename ACC>
__device__ __forceinline__ void vt_add(VertexTable<ACC> &t, int vid, float a0, float a1, float a2, ACC *gout) {
    int slot = (vid * 0x9E3779B1u) >> 25;  // top 7 bits: 0 .. VT_SLOTS-1
    bool done = false;
    for (int probe = 0; probe < 16 && !done; probe++) {
        const int old = atomicCAS(&t.key[slot], -1, vid);
        if (old == -1 || old == vid) {
            lds_add(&t.val[slot][0], a0);
            lds_add(&t.val[slot][1], a1);
            lds_add(&t.val[slot][2], a2);
            done = true;
        }
        slot = (slot + 1) & (VT_SLOTS - 1);
    }
    if (!done) {  // crowded table (many distinct vertices in one tile): straight to memory
        ACC *dst = gout + (size_t)vid * 3;
        acc_add(dst + 0, a0);
        acc_add(dst + 1, a1);
        acc_add(dst + 2, a2);
    }
}

template <typename ACC>
__device__ __forceinline__ void vt_flush(VertexTable<ACC> &t, int lane, ACC *gout) {
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < VT_SLOTS; i += 64) {
        const int key = t.key[i];
        if (key >= 0) {
            ACC *dst = gout + (size_t)key * 3;
            acc_add(dst + 0, t.val[i][0]);
            acc_add(dst + 1, t.val[i][1]);
            acc_add(dst + 2, t.val[i][2]);
        }
    }
}

// Vertex i of [B * N]: (g_u, g_v, g_z) of the projected vertex, summed in gacc (or as fixed point in
// gfix when that is given), becomes the gradient w.r.t. camera xyz, in place in gacc.
__device__ __forceinline__ void project_backward_vertex(const float *verts, float *gacc, const long long *gfix,
                                                        const Cam &cam, long i) {
    const float *q = verts + i * 3;
    float *g = gacc + i * 3;
    float gx, gy, gz;
    if (gfix) {
        const long long *f = gfix + i * 3;
        project_backward(q[0], q[1], q[2], cam, from_fix(f[0]), from_fix(f[1]), from_fix(f[2]), gx, gy, gz);
    } else {
        project_backward(q[0], q[1], q[2], cam, g[0], g[1], g[2], gx, gy, gz);
    }
    g[0] = gx;
    g[1] = gy;
    g[2] = gz;
}

static int make_cam(const float *K, float orig_size, Cam &c) {
    G2S_REQUIRE(K != nullptr, "K must be a host pointer to 9 floats");
    G2S_REQUIRE(K[6] == 0.0f && K[7] == 0.0f && K[8] == 1.0f, "K third row must be 0 0 1");
    c = Cam{K[0], K[1], K[2], K[3], K[4], K[5], orig_size};
    return G2S_OK;
}

}  // namespace g2s
