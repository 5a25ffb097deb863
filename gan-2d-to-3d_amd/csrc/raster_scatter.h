// raster_scatter.h — gradient scatter shared by the rasterizer's backward passes (raster.hip: depth,
// raster_rgb.hip: texture lookup, face_light.hip: per-face light).  The first two run one wave per
// 8x8-sample tile, lane = raster sample, and end the same way: neighbouring samples of one face merge
// their partial sums through shuffles, the per-vertex partials of a tile meet in a per-wave LDS table
// keyed by vertex id, each distinct vertex reaches memory once, and one thread per vertex maps
// (g_u, g_v, g_z) of the projected vertex back to camera xyz (scatter_project).  All three start with
// the same host prologue (scatter_begin: float accumulators, or 2^-40 fixed point in deterministic
// mode, cleared unless the caller did) and turn fixed-point sums back with scatter_unfix.  HIP only.
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

// One thread per vertex i of [B * N]: (g_u, g_v, g_z) of the projected vertex, summed in gacc (or as fixed
// point in gfix when that is given), becomes the gradient w.r.t. camera xyz, in place in gacc.
static __global__ __launch_bounds__(256) void scatter_project(const float *verts, float *gacc, const long long *gfix,
                                                              Cam cam, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
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

// Fixed-point sums back to float: out = fix, or out += fix for a target that already holds a gradient (ADD).
template <bool ADD>
__global__ __launch_bounds__(256) void scatter_unfix(const long long *fix, float *out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = from_fix(fix[i]);
    out[i] = ADD ? out[i] + s : s;
}

static int make_cam(const float *K, float orig_size, Cam &c) {
    G2S_REQUIRE(K != nullptr, "K must be a host pointer to 9 floats");
    G2S_REQUIRE(K[6] == 0.0f && K[7] == 0.0f && K[8] == 1.0f, "K third row must be 0 0 1");
    c = Cam{K[0], K[1], K[2], K[3], K[4], K[5], orig_size};
    return G2S_OK;
}

// One float gradient a backward scatters into: n elements at ptr (ptr may be NULL: not wanted in default mode;
// its n still counts in the fixed-point layout), `name` as the messages call it.
struct ScatterTarget {
    float *ptr;
    size_t n;
    const char *name;
};

// Host prologue of a scattering backward: the accumulators start at zero.  acc_is_zero is the caller's promise that
// they already are (include/g2s.h), and then nothing is cleared.
//   deterministic mode   float atomics would make the sums depend on the order the waves finish in: `fix` becomes the
//                        256-aligned start of `workspace`, which must hold `need` bytes (`sizer`_workspace_bytes is
//                        the query that says so) and takes the targets' sums back to back as 2^-40 fixed point;
//   default mode         `fix` is NULL and the targets themselves are the accumulators.
static int scatter_begin(const char *sizer, size_t need, void *workspace, size_t workspace_bytes, int acc_is_zero,
                         hipStream_t st, const ScatterTarget *targets, int n_targets, long long *&fix) {
    fix = nullptr;
    if (deterministic()) {
        if (!workspace || workspace_bytes < need)
            return fail(G2S_ERR_WORKSPACE, "deterministic mode: the backward needs its fixed-point workspace "
                        "(%s_workspace_bytes = %zu bytes, got %zu)", sizer, need,
                        workspace ? workspace_bytes : (size_t)0);
        fix = reinterpret_cast<long long *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
        size_t total = 0;
        for (int k = 0; k < n_targets; k++) total += targets[k].n;
        if (!acc_is_zero && hipMemsetAsync(fix, 0, total * sizeof(long long), st) != hipSuccess)
            return fail(G2S_ERR_LAUNCH, "hipMemsetAsync(workspace) failed");
    } else if (!acc_is_zero) {
        for (int k = 0; k < n_targets; k++)
            if (targets[k].ptr && hipMemsetAsync(targets[k].ptr, 0, targets[k].n * sizeof(float), st) != hipSuccess)
                return fail(G2S_ERR_LAUNCH, "hipMemsetAsync(%s) failed", targets[k].name);
    }
    return G2S_OK;
}

}  // namespace g2s
