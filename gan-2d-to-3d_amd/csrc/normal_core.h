// normal_core.h — the 3-vector helpers and the back-projected point behind the normals of a depth map
// (renderer.py:127-139), shared by geometry.hip (g2s_normal_*) and metrics.hip (g2s_depth_metrics).
#pragma once
#include <hip/hip_runtime.h>

namespace g2s {

constexpr float NORMAL_EPS = 1e-7f;

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// depth dd of a pixel times its ray r = K^-1 (x, y, 1)
__device__ __forceinline__ V3 pt3_ray(float dd, const float *r) { return V3{r[0] * dd, r[1] * dd, r[2] * dd}; }

__device__ __forceinline__ V3 pt3(const float *d, const float *rays, int W, int y, int x) {
    return pt3_ray(d[y * W + x], rays + 3 * (y * W + x));
}

// un-normalised normal of an interior pixel from the points right, left, below, above it
__device__ __forceinline__ V3 normal_raw(V3 right, V3 left, V3 below, V3 above) {
    return cross3(sub3(right, left), sub3(below, above));
}

// n / (|n| + NORMAL_EPS)
__device__ __forceinline__ V3 normalize_eps(V3 n) {
    const float inv = 1.0f / (sqrtf(n.x * n.x + n.y * n.y + n.z * n.z) + NORMAL_EPS);
    return V3{n.x * inv, n.y * inv, n.z * inv};
}

}  // namespace g2s
