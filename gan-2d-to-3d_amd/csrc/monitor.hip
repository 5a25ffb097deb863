// monitor.hip — the two kernels of training-time monitoring (monitor.py): the sample grid and the latents of the
// perceptual path length.  Both are memory- and launch-bound single launches without atomics, LDS or workspace; every
// output element is written exactly once from the inputs alone, so neither needs a cleared output, both can be
// captured, and two calls give the same bits in every mode of g2s_set_deterministic.
//
//   image_grid_kernel<PX>  torchvision's make_grid + save_image(normalize=True) up to its uint8:
//                          x [N, C, H, W] f32, C in {1, 3} -> out [Hg, Wg, 3] u8.  Threads are laid out over OUTPUT
//                          pixels; each finds the cell it lies in, reads its 1 or 3 channel values (or takes the pad
//                          byte) and quantises with the arithmetic of generate._quantise_torch,
//                              u = (clamp(v, lo, hi) - lo) / max(hi - lo, 1e-5);  uint8(clamp(u * 255 + 0.5, 0, 255)),
//                          every step rounded to f32 (this file is built with -ffp-contract=off).  PX = 4: a thread owns
//                          four consecutive pixels of one row and stores their 12 bytes as three dwords (Wg % 4 == 0
//                          and a 4-byte aligned output; a wave then writes 768 contiguous bytes).  The reads stay
//                          dwords: a cell starts `padding` columns into its group, so the four source floats of a
//                          thread are in general neither aligned nor from one image; across a wave they are still
//                          contiguous runs of each image row.  PX = 1 otherwise (byte stores).
//   ppl_latents_kernel<V, NCH>
//                          one 64-lane wave per pair (a, b) = rows 2i, 2i + 1 of `pairs` [2B, D]; both output rows
//                          (the point at t[i] and the one at t1 = t[i] + eps, the sum rounded to f32) come from ONE
//                          read of the pair, kept in registers (NCH chunks of V floats per lane; V = 4: 16-byte loads
//                          and stores when D % 4 == 0 and the bases are aligned).  NCH = 0 is the form for any D: the
//                          pair is read again, from L2, by each pass.
//                            mode 0 (w):  a + (b - a) * t
//                            mode 1 (z):  slerp.  a^ = a / |a|, b^ = b / |b|, d = <a^, b^>, p = t * acos(d),
//                                         c = (b^ - d a^) / |b^ - d a^|, out = n(a^ cos p + c sin p).
//                          The sums (|a|^2, |b|^2, <a, b>; |b^ - d a^|^2; the two output norms) are butterflies of
//                          wave_sum.h over per-lane partial sums taken in ascending chunk order: a fixed order, the
//                          same bits on every run.  All arithmetic between the load and the store is in double: the
//                          launch is bound by its latency, not by the 2 D values per pair, and acos near d = 1
//                          (nearly parallel ends) and the cancellation in b^ - d a^ then cost nothing at f32 output.
#include "g2s_common.h"
#include "wave_sum.h"

namespace g2s {

// ------------------------------------------------------------------------------------------------------- the grid
struct GridParams {
    const float *x;
    uint8_t *out;
    int N, C, H, W;
    int xmaps, ymaps, Hg, Wg, padding, bare;     // bare: N == 1, the image without a border
    float lo, hi, den;                            // den = max(hi - lo, 1e-5)
    unsigned pad_byte;
};

__device__ __forceinline__ unsigned grid_quantise(float v, float lo, float hi, float den) {
    v = fminf(fmaxf(v, lo), hi);
    v = (v - lo) / den;
    v = v * 255.0f + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (unsigned)(int)v;
}

// the three bytes of output pixel (y, x) as r | g << 8 | b << 16
__device__ __forceinline__ unsigned grid_pixel(const GridParams &p, int y, int x) {
    int k = 0, iy = y, ix = x;
    if (!p.bare) {
        const int ch = p.H + p.padding, cw = p.W + p.padding;
        const int cy = y / ch, cx = x / cw;
        iy = y - cy * ch - p.padding, ix = x - cx * cw - p.padding;
        k = cy * p.xmaps + cx;
        // the border rows and columns, the last border (cy == ymaps / cx == xmaps) and the cells after the last image
        if (iy < 0 || ix < 0 || cy >= p.ymaps || cx >= p.xmaps || k >= p.N) return p.pad_byte * 0x010101u;
    }
    const long HW = (long)p.H * p.W;
    const float *src = p.x + (long)k * p.C * HW + (long)iy * p.W + ix;
    const unsigned r = grid_quantise(src[0], p.lo, p.hi, p.den);
    if (p.C == 1) return r * 0x010101u;
    const unsigned g = grid_quantise(src[HW], p.lo, p.hi, p.den);
    const unsigned b = grid_quantise(src[2 * HW], p.lo, p.hi, p.den);
    return r | (g << 8) | (b << 16);
}

template <int PX>
__global__ __launch_bounds__(256) void image_grid_kernel(GridParams p) {
    const long total = (long)p.Hg * p.Wg;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * PX;      // first output pixel of this thread
    if (i >= total) return;
    const int y = (int)(i / p.Wg), x = (int)(i - (long)y * p.Wg);
    if (PX == 4) {      // Wg % 4 == 0: the four pixels are in row y; 3 i is a multiple of 4
        const unsigned q0 = grid_pixel(p, y, x), q1 = grid_pixel(p, y, x + 1), q2 = grid_pixel(p, y, x + 2),
                       q3 = grid_pixel(p, y, x + 3);
        uint32_t *dst = reinterpret_cast<uint32_t *>(p.out + i * 3);
        dst[0] = q0 | (q1 << 24);
        dst[1] = (q1 >> 8) | (q2 << 16);
        dst[2] = (q2 >> 16) | (q3 << 8);
    } else {
        const unsigned q = grid_pixel(p, y, x);
        uint8_t *dst = p.out + i * 3;
        dst[0] = (uint8_t)q, dst[1] = (uint8_t)(q >> 8), dst[2] = (uint8_t)(q >> 16);
    }
}

// ---------------------------------------------------------------------------------------------- path-length latents
constexpr int PL_WAVES = 4;     // pairs per workgroup

typedef float pl_v4 __attribute__((ext_vector_type(4)));

struct PplParams {
    const float *pairs, *t;
    float *out;
    float eps;
    int mode, B, D;
};

template <int V> struct PlVec;
template <> struct PlVec<1> { typedef float type; };
template <> struct PlVec<4> { typedef pl_v4 type; };

template <int V> __device__ __forceinline__ float pl_get(const typename PlVec<V>::type &v, int e);
template <> __device__ __forceinline__ float pl_get<1>(const float &v, int) { return v; }
template <> __device__ __forceinline__ float pl_get<4>(const pl_v4 &v, int e) { return v[e]; }
template <int V> __device__ __forceinline__ void pl_set(typename PlVec<V>::type &v, int e, float s);
template <> __device__ __forceinline__ void pl_set<1>(float &v, int, float s) { v = s; }
template <> __device__ __forceinline__ void pl_set<4>(pl_v4 &v, int e, float s) { v[e] = s; }

// NCH > 0: D <= 64 * V * NCH and the pair stays in registers; NCH == 0: any D, every pass reads the pair again.
template <int V, int NCH>
__global__ __launch_bounds__(64 * PL_WAVES) void ppl_latents_kernel(PplParams p) {
    typedef typename PlVec<V>::type T;
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * PL_WAVES + (threadIdx.x >> 6);
    if (pair >= p.B) return;        // a whole wave leaves: the butterflies below see 64 live lanes
    const int units = p.D / V;      // V == 4 only when D % 4 == 0
    const int chunks = NCH > 0 ? NCH : (units + 63) / 64;
    const T *A = reinterpret_cast<const T *>(p.pairs + (long)(2 * pair) * p.D);
    const T *Bv = reinterpret_cast<const T *>(p.pairs + (long)(2 * pair + 1) * p.D);
    T *O0 = reinterpret_cast<T *>(p.out + (long)(2 * pair) * p.D);
    T *O1 = reinterpret_cast<T *>(p.out + (long)(2 * pair + 1) * p.D);
    const float tf = p.t[pair];
    const float t1f = tf + p.eps;       // rounded to f32: the t1 of a float32 tensor add
    const double t0 = (double)tf, t1 = (double)t1f;

    constexpr int KEEP = NCH > 0 ? NCH : 1;
    T ra[KEEP], rb[KEEP];
    if (NCH > 0) {
#pragma unroll
        for (int j = 0; j < KEEP; j++) {
            const int u = j * 64 + lane;
            if (u < units) ra[j] = A[u], rb[j] = Bv[u];
        }
    }
#define PL_FOR_EACH(...)                                                              \
    if (NCH > 0) {                                                                      \
        _Pragma("unroll") for (int j = 0; j < KEEP; j++) {                              \
            const int u = j * 64 + lane;                                                \
            if (u < units) { const T va = ra[j], vb = rb[j]; __VA_ARGS__ }                     \
        }                                                                               \
    } else {                                                                            \
        for (int j = 0; j < chunks; j++) {                                              \
            const int u = j * 64 + lane;                                                \
            if (u < units) { const T va = A[u], vb = Bv[u]; __VA_ARGS__ }                      \
        }                                                                               \
    }

    if (p.mode == 0) {
        PL_FOR_EACH({
            T o0, o1;
            for (int e = 0; e < V; e++) {
                const double a = pl_get<V>(va, e), b = pl_get<V>(vb, e);
                pl_set<V>(o0, e, (float)(a + (b - a) * t0));
                pl_set<V>(o1, e, (float)(a + (b - a) * t1));
            }
            O0[u] = o0, O1[u] = o1;
        })
        return;
    }

    double saa = 0.0, sbb = 0.0, sab = 0.0;
    PL_FOR_EACH({
        for (int e = 0; e < V; e++) {
            const double a = pl_get<V>(va, e), b = pl_get<V>(vb, e);
            saa += a * a, sbb += b * b, sab += a * b;
        }
    })
    saa = wave_sum(saa), sbb = wave_sum(sbb), sab = wave_sum(sab);
    const double ia = 1.0 / sqrt(saa), ib = 1.0 / sqrt(sbb);
    const double d = sab * ia * ib;
    double scc = 0.0;
    PL_FOR_EACH({
        for (int e = 0; e < V; e++) {
            const double a = pl_get<V>(va, e) * ia, b = pl_get<V>(vb, e) * ib;
            const double c = b - d * a;
            scc += c * c;
        }
    })
    scc = wave_sum(scc);
    const double ic = 1.0 / sqrt(scc);
    const double om = acos(d);
    const double c0 = cos(t0 * om), s0 = sin(t0 * om), c1 = cos(t1 * om), s1 = sin(t1 * om);
    double sr0 = 0.0, sr1 = 0.0;
    PL_FOR_EACH({
        for (int e = 0; e < V; e++) {
            const double a = pl_get<V>(va, e) * ia, b = pl_get<V>(vb, e) * ib;
            const double c = (b - d * a) * ic;
            const double r0 = a * c0 + c * s0, r1 = a * c1 + c * s1;
            sr0 += r0 * r0, sr1 += r1 * r1;
        }
    })
    sr0 = wave_sum(sr0), sr1 = wave_sum(sr1);
    const double i0 = 1.0 / sqrt(sr0), i1 = 1.0 / sqrt(sr1);
    PL_FOR_EACH({
        T o0, o1;
        for (int e = 0; e < V; e++) {
            const double a = pl_get<V>(va, e) * ia, b = pl_get<V>(vb, e) * ib;
            const double c = (b - d * a) * ic;
            pl_set<V>(o0, e, (float)((a * c0 + c * s0) * i0));
            pl_set<V>(o1, e, (float)((a * c1 + c * s1) * i1));
        }
        O0[u] = o0, O1[u] = o1;
    })
#undef PL_FOR_EACH
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_image_grid_u8(const float *x, uint8_t *out, int N, int C, int H, int W, int nrow, int padding,
                                 float lo, float hi, float pad_value, g2s_stream_t stream) {
    const char *what = "g2s_image_grid_u8";
    G2S_REQUIRE(x && out, "%s: NULL pointer", what);
    G2S_REQUIRE(N >= 1 && H >= 1 && W >= 1 && nrow >= 1, "%s: N, H, W and nrow must be positive", what);
    G2S_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3, got %d", what, C);
    G2S_REQUIRE(padding >= 0, "%s: padding must be >= 0", what);
    G2S_REQUIRE(lo == lo && hi == hi && pad_value == pad_value, "%s: lo, hi and pad_value must not be NaN", what);
    GridParams p;
    p.x = x, p.out = out, p.N = N, p.C = C, p.H = H, p.W = W, p.padding = padding;
    p.bare = N == 1;
    p.xmaps = nrow < N ? nrow : N;
    p.ymaps = (N + p.xmaps - 1) / p.xmaps;
    const long Hg = p.bare ? H : (long)p.ymaps * ((long)H + padding) + padding;
    const long Wg = p.bare ? W : (long)p.xmaps * ((long)W + padding) + padding;
    G2S_REQUIRE(Hg * Wg < (1l << 31) && Hg < (1l << 31) && Wg < (1l << 31), "%s: the grid has 2^31 pixels or more", what);
    G2S_REQUIRE((long)N * C * H * W < (1l << 40), "%s: input too large", what);
    p.Hg = (int)Hg, p.Wg = (int)Wg;
    p.lo = lo, p.hi = hi;
    p.den = fmaxf(hi - lo, 1e-5f);
    p.pad_byte = (unsigned)(int)fminf(fmaxf(pad_value * 255.0f + 0.5f, 0.0f), 255.0f);
    const long total = Hg * Wg;
    if (Wg % 4 == 0 && ((uintptr_t)out & 3) == 0)
        image_grid_kernel<4><<<cdiv(total / 4, 256), 256, 0, as_stream(stream)>>>(p);
    else
        image_grid_kernel<1><<<cdiv(total, 256), 256, 0, as_stream(stream)>>>(p);
    return check_launch(what);
}

extern "C" int g2s_ppl_latents(const float *pairs, const float *t, float eps, int mode, float *out, int B, int D,
                               g2s_stream_t stream) {
    const char *what = "g2s_ppl_latents";
    G2S_REQUIRE(pairs && t && out, "%s: NULL pointer", what);
    G2S_REQUIRE(B >= 1 && D >= 1, "%s: B and D must be positive", what);
    G2S_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (w, lerp) or 1 (z, slerp), got %d", what, mode);
    G2S_REQUIRE(eps == eps, "%s: eps must not be NaN", what);
    G2S_REQUIRE(2l * B * D < (1l << 40) && B <= (1 << 30), "%s: too many values", what);
    const uintptr_t pa = (uintptr_t)pairs, oa = (uintptr_t)out, bytes = (uintptr_t)2 * B * D * sizeof(float);
    G2S_REQUIRE(pa + bytes <= oa || oa + bytes <= pa, "%s: out overlaps pairs", what);
    PplParams p;
    p.pairs = pairs, p.t = t, p.out = out, p.eps = eps, p.mode = mode, p.B = B, p.D = D;
    const dim3 grid((unsigned)cdiv(B, PL_WAVES));
    const int threads = 64 * PL_WAVES;
    hipStream_t st = as_stream(stream);
    // rows start at multiples of D floats: 16-byte accesses need D % 4 == 0 and aligned bases
    const bool wide = D % 4 == 0 && (((uintptr_t)pairs | (uintptr_t)out) & 15) == 0;
    if (wide && D <= 256) ppl_latents_kernel<4, 1><<<grid, threads, 0, st>>>(p);
    else if (wide && D <= 512) ppl_latents_kernel<4, 2><<<grid, threads, 0, st>>>(p);
    else if (wide) ppl_latents_kernel<4, 0><<<grid, threads, 0, st>>>(p);
    else if (D <= 128) ppl_latents_kernel<1, 2><<<grid, threads, 0, st>>>(p);
    else ppl_latents_kernel<1, 0><<<grid, threads, 0, st>>>(p);
    return check_launch(what);
}
