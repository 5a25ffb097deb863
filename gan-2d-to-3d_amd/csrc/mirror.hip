// mirror.hip — the symmetry pair of a flipped step (model.py forward_step1 / forward_step3 with flip1 / flip3):
// x [N, C, H, W], repeat >= 1  ->  y [2 N repeat, C, H, W]: row n * repeat + r is x[n], row N * repeat + n * repeat + r
// is x[n] mirrored along W.  One launch serves the depth (C = 1) and the albedo (C = 3) of a step; the backward is
// a gather over the 2 * repeat output rows of every input element in one fixed order (no atomics: bit-reproducible).
//
// A work unit is one float4 of an input row (W % 4 == 0, both pointers 16-byte aligned: every row then starts on a
// 16-byte boundary) or one float.  The mirror of the float4 at column quad q is the reversed float4 at quad
// W / 4 - 1 - q, so both halves are written (forward) and read (backward) as whole 16-byte accesses.
#include "g2s_common.h"

namespace g2s {

constexpr int MP_THREADS = 256;
constexpr int MP_MAX_BLOCKS = 2048;     // memory-bound: cap the grid and stride over the rest

typedef float mp_v4 __attribute__((ext_vector_type(4)));

struct MirrorTensor {
    const float *in;    // forward: x; backward: gy
    float *out;         // forward: y; backward: gx
    long units;         // N * CH * (vec ? W / 4 : W), 0 for an absent tensor
    int CH;             // C * H rows of W per sample
    int vec;
};

struct MirrorParams {
    MirrorTensor t[2];
    int N, W, repeat;
};

__device__ inline mp_v4 mp_rev(mp_v4 v) { return mp_v4{v.w, v.z, v.y, v.x}; }

template <typename T> __device__ inline T mp_mirror(T v);
template <> __device__ inline float mp_mirror<float>(float v) { return v; }
template <> __device__ inline mp_v4 mp_mirror<mp_v4>(mp_v4 v) { return mp_rev(v); }

// unit u of tensor t -> sample n, row ch, column unit q (of Wu per row); out-row stride of one sample: CH * Wu
template <typename T, bool BWD>
__device__ inline void mp_unit(const MirrorTensor &t, long u, int N, int Wu, int repeat) {
    const long per = (long)t.CH * Wu;           // units of one sample
    const int n = (int)(u / per);
    const long in_row = u - (long)n * per;      // ch * Wu + q
    const int q = (int)(in_row % Wu);
    const long mir_row = in_row - q + (Wu - 1 - q);
    const long plain0 = (long)n * repeat * per;                       // sample row n * repeat
    const long mirr0 = ((long)N * repeat + (long)n * repeat) * per;   // sample row N * repeat + n * repeat
    if (!BWD) {
        const T *x = reinterpret_cast<const T *>(t.in);
        T *y = reinterpret_cast<T *>(t.out);
        const T v = x[u];
        const T m = mp_mirror<T>(v);
        for (int r = 0; r < repeat; r++) {
            y[plain0 + r * per + in_row] = v;
            y[mirr0 + r * per + mir_row] = m;
        }
    } else {
        const T *gy = reinterpret_cast<const T *>(t.in);
        T *gx = reinterpret_cast<T *>(t.out);
        // fixed order: the plain rows r = 0 .. repeat - 1, then the mirrored rows r = 0 .. repeat - 1
        T acc = gy[plain0 + in_row];
        for (int r = 1; r < repeat; r++) acc += gy[plain0 + r * per + in_row];
        for (int r = 0; r < repeat; r++) acc += mp_mirror<T>(gy[mirr0 + r * per + mir_row]);
        gx[u] = acc;
    }
}

template <bool BWD>
__global__ __launch_bounds__(MP_THREADS) void mirror_pair_kernel(MirrorParams p) {
    const long total = p.t[0].units + p.t[1].units;
    const long stride = (long)gridDim.x * MP_THREADS;
    for (long u = (long)blockIdx.x * MP_THREADS + threadIdx.x; u < total; u += stride) {
        const bool second = u >= p.t[0].units;
        const MirrorTensor &t = p.t[second ? 1 : 0];
        const long v = second ? u - p.t[0].units : u;
        if (t.vec) mp_unit<mp_v4, BWD>(t, v, p.N, p.W / 4, p.repeat);
        else mp_unit<float, BWD>(t, v, p.N, p.W, p.repeat);
    }
}

static int mirror_launch(bool bwd, const char *what, const float *in0, float *out0, int C0, const float *in1,
                         float *out1, int C1, int N, int H, int W, int repeat, g2s_stream_t stream) {
    G2S_REQUIRE(in0 && out0 && C0 > 0, "%s: the first tensor is required", what);
    G2S_REQUIRE((in1 != nullptr) == (out1 != nullptr) && (in1 != nullptr) == (C1 > 0),
                "%s: the second tensor is given whole (both pointers, C1 > 0) or not at all (NULL, NULL, 0)", what);
    G2S_REQUIRE(N > 0 && H > 0 && W > 0 && repeat > 0, "%s: N, H, W, repeat must be positive", what);
    MirrorParams p;
    p.N = N, p.W = W, p.repeat = repeat;
    const float *ins[2] = {in0, in1};
    float *outs[2] = {out0, out1};
    const int Cs[2] = {C0, C1};
    for (int i = 0; i < 2; i++) {
        MirrorTensor &t = p.t[i];
        t.in = ins[i], t.out = outs[i];
        const long big = 2l * N * repeat * Cs[i] * H * (long)W;      // elements of the wide side
        G2S_REQUIRE(big < (1l << 40), "%s: tensor too large", what);
        G2S_REQUIRE((long)Cs[i] * H < (1l << 31), "%s: C * H too large", what);
        t.CH = Cs[i] * H;
        t.vec = ins[i] && W % 4 == 0 && ((uintptr_t)ins[i] | (uintptr_t)outs[i]) % 16 == 0;
        t.units = ins[i] ? (long)N * t.CH * (t.vec ? W / 4 : W) : 0;
    }
    const long total = p.t[0].units + p.t[1].units;
    const int blocks = (int)((total + MP_THREADS - 1) / MP_THREADS < MP_MAX_BLOCKS ? (total + MP_THREADS - 1) / MP_THREADS
                                                                                  : MP_MAX_BLOCKS);
    if (bwd) mirror_pair_kernel<true><<<blocks, MP_THREADS, 0, as_stream(stream)>>>(p);
    else mirror_pair_kernel<false><<<blocks, MP_THREADS, 0, as_stream(stream)>>>(p);
    return check_launch(what);
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_mirror_pair_fwd(const float *x0, float *y0, int C0, const float *x1, float *y1, int C1, int N, int H,
                                   int W, int repeat, g2s_stream_t stream) {
    return mirror_launch(false, "g2s_mirror_pair_fwd", x0, y0, C0, x1, y1, C1, N, H, W, repeat, stream);
}

extern "C" int g2s_mirror_pair_bwd(const float *gy0, float *gx0, int C0, const float *gy1, float *gx1, int C1, int N,
                                   int H, int W, int repeat, g2s_stream_t stream) {
    return mirror_launch(true, "g2s_mirror_pair_bwd", gy0, gx0, C0, gy1, gx1, C1, N, H, W, repeat, stream);
}
