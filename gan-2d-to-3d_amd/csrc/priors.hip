// priors.hip — the depth priors of the depth-net pre-training (GAN2Shape/priors.py:7-107), batched over
// images and built on the device: no host round trip, no synchronisation, recordable in a HIP graph.
//
//   g2s_prior_map        box / masked_box / confidence: one expression per pixel       (priors.py:26-45,99-103)
//   g2s_prior_smooth     passes x (valid box filter, rescale to [near, far], far border) (priors.py:47-67)
//   g2s_prior_ellipsoid  spherical cap over the bounding box of mask >= threshold        (priors.py:74-97)
//
// The arithmetic restates the torch expressions operation by operation in fp32 (this file is compiled
// with -ffp-contract=off), with the host scalars rounded to fp32 where torch rounds them.  Every image
// of the batch is independent: each min / max / bounding box is per image.
//
// Smoothing.  A pass is two launches: row sums (taps consecutive inputs, left to right), then column
// sums of those (top to bottom) times 1/taps — every output is summed directly, in one fixed order, so
// the rounding error does not grow with S.  The column kernel also reduces the per-image min and max of
// the filtered map: in the wave, in the workgroup, then one unsigned atomic max per workgroup on an
// order-preserving integer encoding of the float (the min as the max of the complement).  min and max
// are exact and order-independent, hence the result is bit-reproducible whatever the deterministic flag
// says.  The rescale of pass k is applied by whoever reads its map next (the row kernel of pass k + 1,
// or the final kernel that writes `out`): the dependency between passes never leaves the device.
#include "g2s_common.h"

namespace g2s {

// ------------------------------------------------------------------ map priors
struct MapArgs {
    float t, inv, far;          // fp32(threshold), fp32(1 - threshold), fp32(far)
    int r0, r1, c0, c1;         // the box of `box`
};

// grid (ceil(S*S / 256), B)
__global__ __launch_bounds__(256) void prior_map_kernel(const float *__restrict__ mask, float *__restrict__ out,
                                                        int S, int kind, MapArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S * S) return;
    const size_t i = (size_t)blockIdx.y * S * S + p;
    float v;
    if (kind == 0) {
        const int y = p / S, x = p - y * S;
        v = (y >= a.r0 && y < a.r1 && x >= a.c0 && x < a.c1) ? 1.0f : 0.0f;
    } else if (kind == 1) {
        float m = mask[i];
        m = (m < a.t) ? 0.0f : m;
        v = a.far - a.far * ((m - a.t) / a.inv);
    } else {
        v = a.far - a.far * mask[i];
    }
    out[i] = v;
}

// ------------------------------------------------------------------ smoothing
// Order-preserving map float -> uint32 (a < b  <=>  enc(a) < enc(b), -0 < +0) and back.
__device__ __forceinline__ unsigned enc_ordered(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_ordered(unsigned e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

struct Rescale { float near, far, range; };   // range = fp32(far - near)

// Value at (y, x) of the S x S map a pass hands to the next one: `far` on the border of width h, else
// near + (f - lo) * range / (hi - lo) of the V x V filtered map f, with d = hi - lo taken once per thread.
// d == 0 (a constant filtered map, where the host expression is 0 / 0): `near`.
__device__ __forceinline__ float rescaled(const float *__restrict__ f, int y, int x, int V, int h, float lo,
                                          float d, Rescale r) {
    if (y < h || y >= h + V || x < h || x >= h + V) return r.far;
    if (d == 0.0f) return r.near;
    return r.near + (f[(y - h) * V + (x - h)] - lo) * r.range / d;
}

// Row sums: rows[b][y][x] = sum_{j < taps} in(y, x + j), y < S, x < V.  `slot` == nullptr: `src` is the
// S x S input of the first pass; else `src` is the previous pass's V x V filtered map and slot[2 b],
// slot[2 b + 1] hold its ~enc(min), enc(max).  grid (ceil(S*V / 256), B)
__global__ __launch_bounds__(256) void smooth_rows_kernel(const float *__restrict__ src,
                                                          const unsigned *__restrict__ slot,
                                                          float *__restrict__ rows, int S, int V, int taps,
                                                          Rescale r) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S * V) return;
    const int b = blockIdx.y, y = p / V, x = p - y * V;
    float acc;
    if (slot == nullptr) {
        const float *in = src + (size_t)b * S * S + (size_t)y * S + x;
        acc = in[0];
        for (int j = 1; j < taps; ++j) acc += in[j];
    } else {
        const float *f = src + (size_t)b * V * V;
        const float lo = dec_ordered(~slot[2 * b]), hi = dec_ordered(slot[2 * b + 1]);
        const int h = taps / 2;
        const float d = hi - lo;
        acc = rescaled(f, y, x, V, h, lo, d, r);
        for (int j = 1; j < taps; ++j) acc += rescaled(f, y, x + j, V, h, lo, d, r);
    }
    rows[(size_t)b * S * V + p] = acc;
}

// Column sums: f[b][y][x] = (sum_{i < taps} rows[b][y + i][x]) * w, y, x < V, and the per-image min / max
// of f into slot[2 b], slot[2 b + 1] (zero-initialised by the launcher).  grid (ceil(V*V / 256), B)
__global__ __launch_bounds__(256) void smooth_cols_kernel(const float *__restrict__ rows, float *__restrict__ f,
                                                          unsigned *__restrict__ slot, int S, int V, int taps,
                                                          float w) {
    __shared__ unsigned red[8];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    unsigned nmin = 0u, vmax = 0u;     // ~enc(+inf-most) and enc(-inf-most): neutral for an unsigned max
    if (p < V * V) {
        const int y = p / V, x = p - y * V;
        const float *in = rows + (size_t)b * S * V + (size_t)y * V + x;
        float acc = in[0];
        for (int i = 1; i < taps; ++i) acc += in[(size_t)i * V];
        const float v = acc * w;
        f[(size_t)b * V * V + p] = v;
        vmax = enc_ordered(v);
        nmin = ~vmax;
    }
    for (int o = 32; o > 0; o >>= 1) {
        nmin = max(nmin, (unsigned)__shfl_xor((int)nmin, o));
        vmax = max(vmax, (unsigned)__shfl_xor((int)vmax, o));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[2 * wave] = nmin; red[2 * wave + 1] = vmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(slot + 2 * b, max(max(red[0], red[2]), max(red[4], red[6])));
        atomicMax(slot + 2 * b + 1, max(max(red[1], red[3]), max(red[5], red[7])));
    }
}

// out = the rescaled, re-bordered map of the last pass.  grid (ceil(S*S / 256), B)
__global__ __launch_bounds__(256) void smooth_final_kernel(const float *__restrict__ f,
                                                           const unsigned *__restrict__ slot,
                                                           float *__restrict__ out, int S, int V, int taps,
                                                           Rescale r) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S * S) return;
    const int b = blockIdx.y, y = p / S, x = p - y * S;
    const float lo = dec_ordered(~slot[2 * b]), hi = dec_ordered(slot[2 * b + 1]);
    out[(size_t)b * S * S + p] = rescaled(f + (size_t)b * V * V, y, x, V, taps / 2, lo, hi - lo, r);
}

// ------------------------------------------------------------------ ellipsoid
// box[4 b ..] = (max_y, min_y, max_x, min_x) of mask >= t over image b; max < min when no pixel
// qualifies.  One workgroup of 1024 threads per image, integer min / max only.
__global__ __launch_bounds__(1024) void mask_box_kernel(const float *__restrict__ mask, int *__restrict__ box,
                                                        int S, float t) {
    __shared__ int red[16 * 4];
    const int b = blockIdx.x;
    const float *m = mask + (size_t)b * S * S;
    int y1 = -1, y0 = S, x1 = -1, x0 = S;
    for (int p = threadIdx.x; p < S * S; p += 1024) {
        if (m[p] >= t) {
            const int y = p / S, x = p - y * S;
            y1 = max(y1, y); y0 = min(y0, y); x1 = max(x1, x); x0 = min(x0, x);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        y1 = max(y1, __shfl_xor(y1, o)); y0 = min(y0, __shfl_xor(y0, o));
        x1 = max(x1, __shfl_xor(x1, o)); x0 = min(x0, __shfl_xor(x0, o));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[4 * wave] = y1; red[4 * wave + 1] = y0; red[4 * wave + 2] = x1; red[4 * wave + 3] = x0; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            y1 = max(y1, red[4 * w]); y0 = min(y0, red[4 * w + 1]);
            x1 = max(x1, red[4 * w + 2]); x0 = min(x0, red[4 * w + 3]);
        }
        box[4 * b] = y1; box[4 * b + 1] = y0; box[4 * b + 2] = x1; box[4 * b + 3] = x0;
    }
}

struct CapArgs { float R, R2, rim, near, far, half_S; };   // fp32 of R, R^2, the rim half-width, S / 2

// grid (ceil(S*S / 256), B)
__global__ __launch_bounds__(256) void ellipsoid_kernel(const int *__restrict__ box, float *__restrict__ out,
                                                        int S, CapArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S * S) return;
    const int b = blockIdx.y, y = p / S, x = p - y * S;
    const int *bx = box + 4 * b;
    const float top = (float)bx[0], bottom = (float)bx[1], right = (float)bx[2], left = (float)bx[3];
    float v = a.far;
    if (bx[0] > bx[1] && bx[2] > bx[3]) {      // else: empty mask, or a box of zero height or width
        const float half_width = (right - left) / 2.0f;
        const float aspect = (top - bottom) / (right - left);
        const float cx = (right + left) / 2.0f, cy = (top + bottom) / 2.0f;
        const float row = ((float)y - a.half_S) / aspect + a.half_S;
        const float dy = row - cy, dx = (float)x - cx;
        const float dist = sqrtf(dy * dy + dx * dx);
        const float rho = dist / half_width * a.rim;
        const float cap = a.R - sqrtf(fabsf(a.R2 - rho * rho)) + a.near;
        if (dist <= half_width) v = cap;
    }
    out[(size_t)b * S * S + p] = v;
}

static const int MAX_S = 2048;
static size_t align256(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_prior_map(const float *mask, int B, int S, int kind, double threshold, double far,
                             float *out, g2s_stream_t stream) {
    G2S_REQUIRE(B >= 0 && B <= 65535, "g2s_prior_map: B = %d out of range", B);
    G2S_REQUIRE(S >= 1 && S <= MAX_S, "g2s_prior_map: S = %d out of range [1, %d]", S, MAX_S);
    G2S_REQUIRE(kind >= 0 && kind <= 2, "g2s_prior_map: kind %d (0 box, 1 masked_box, 2 confidence)", kind);
    G2S_REQUIRE(kind != 1 || (threshold >= 0.0 && threshold < 1.0), "g2s_prior_map: threshold outside [0, 1)");
    if (B == 0) return G2S_OK;
    G2S_REQUIRE(out && (mask || kind == 0), "g2s_prior_map: NULL pointer");
    MapArgs a;
    a.t = (float)threshold;
    a.inv = (float)(1 - threshold);
    a.far = (float)far;
    const int centre = S / 2, half_rows = (int)(S * 0.8 * 0.5), half_cols = (int)(S * 0.5 * 0.5);
    a.r0 = centre - half_rows; a.r1 = centre + half_rows;
    a.c0 = centre - half_cols; a.c1 = centre + half_cols;
    prior_map_kernel<<<dim3(cdiv((long)S * S, 256), B), 256, 0, as_stream(stream)>>>(mask, out, S, kind, a);
    return check_launch("g2s_prior_map");
}

extern "C" size_t g2s_prior_smooth_workspace_bytes(int B, int S, int taps, int passes) {
    if (B <= 0 || S <= 0 || taps <= 0 || taps > S || passes <= 0) return 0;
    const size_t V = (size_t)(S - taps + 1);
    return align256((size_t)B * 2 * passes * sizeof(unsigned)) + align256((size_t)B * S * V * sizeof(float)) +
           align256((size_t)B * V * V * sizeof(float));
}

extern "C" int g2s_prior_smooth(const float *x, int B, int S, int taps, int passes, double near, double far,
                                float *out, void *workspace, size_t workspace_bytes, g2s_stream_t stream) {
    G2S_REQUIRE(B >= 0 && B <= 65535, "g2s_prior_smooth: B = %d out of range", B);
    G2S_REQUIRE(S >= 1 && S <= MAX_S, "g2s_prior_smooth: S = %d out of range [1, %d]", S, MAX_S);
    G2S_REQUIRE(taps >= 1 && (taps & 1) && taps <= S, "g2s_prior_smooth: taps = %d must be odd and <= S = %d", taps, S);
    G2S_REQUIRE(passes >= 0, "g2s_prior_smooth: passes = %d < 0", passes);
    G2S_REQUIRE(near < far, "g2s_prior_smooth: near >= far");
    if (B == 0) return G2S_OK;
    G2S_REQUIRE(x && out, "g2s_prior_smooth: NULL pointer");
    hipStream_t st = as_stream(stream);
    if (passes == 0) {
        if (x != out && hipMemcpyAsync(out, x, (size_t)B * S * S * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(G2S_ERR_LAUNCH, "g2s_prior_smooth: hipMemcpyAsync failed");
        return G2S_OK;
    }
    const size_t need = g2s_prior_smooth_workspace_bytes(B, S, taps, passes);
    if (!workspace || workspace_bytes < need)
        return fail(G2S_ERR_WORKSPACE, "g2s_prior_smooth: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, need);
    const int V = S - taps + 1;
    const size_t slot_bytes = align256((size_t)B * 2 * passes * sizeof(unsigned));
    unsigned *slots = (unsigned *)workspace;
    float *rows = (float *)((char *)workspace + slot_bytes);
    float *f = (float *)((char *)rows + align256((size_t)B * S * V * sizeof(float)));
    if (hipMemsetAsync(slots, 0, (size_t)B * 2 * passes * sizeof(unsigned), st) != hipSuccess)
        return fail(G2S_ERR_LAUNCH, "g2s_prior_smooth: hipMemsetAsync failed");
    const Rescale r{(float)near, (float)far, (float)(far - near)};
    const float w = (float)(1.0 / taps);
    for (int k = 0; k < passes; ++k) {
        // pass k reads f (pass k - 1) through the row kernel before its column kernel overwrites it
        const unsigned *prev = k ? slots + (size_t)(k - 1) * 2 * B : nullptr;
        smooth_rows_kernel<<<dim3(cdiv((long)S * V, 256), B), 256, 0, st>>>(k ? f : x, prev, rows, S, V, taps, r);
        smooth_cols_kernel<<<dim3(cdiv((long)V * V, 256), B), 256, 0, st>>>(rows, f, slots + (size_t)k * 2 * B, S, V, taps, w);
    }
    smooth_final_kernel<<<dim3(cdiv((long)S * S, 256), B), 256, 0, st>>>(f, slots + (size_t)(passes - 1) * 2 * B, out, S, V, taps, r);
    return check_launch("g2s_prior_smooth");
}

extern "C" size_t g2s_prior_ellipsoid_workspace_bytes(int B) {
    return B > 0 ? (size_t)B * 4 * sizeof(int) : 0;
}

extern "C" int g2s_prior_ellipsoid(const float *mask, int B, int S, double threshold, double radius, double near,
                                   double far, float *out, void *workspace, size_t workspace_bytes,
                                   g2s_stream_t stream) {
    G2S_REQUIRE(B >= 0 && B <= 65535, "g2s_prior_ellipsoid: B = %d out of range", B);
    G2S_REQUIRE(S >= 1 && S <= MAX_S, "g2s_prior_ellipsoid: S = %d out of range [1, %d]", S, MAX_S);
    G2S_REQUIRE(near < far, "g2s_prior_ellipsoid: near >= far");
    G2S_REQUIRE(radius > 0.0 && far - near <= 2 * radius, "g2s_prior_ellipsoid: radius must be positive and 2 radius >= far - near");
    if (B == 0) return G2S_OK;
    G2S_REQUIRE(mask && out, "g2s_prior_ellipsoid: NULL pointer");
    const size_t need = g2s_prior_ellipsoid_workspace_bytes(B);
    if (!workspace || workspace_bytes < need)
        return fail(G2S_ERR_WORKSPACE, "g2s_prior_ellipsoid: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = as_stream(stream);
    int *box = (int *)workspace;
    const double d = radius - (far - near);
    const CapArgs a{(float)radius, (float)(radius * radius), (float)sqrt(radius * radius - d * d), (float)near, (float)far, (float)(S / 2.0)};
    mask_box_kernel<<<B, 1024, 0, st>>>(mask, box, S, (float)threshold);
    ellipsoid_kernel<<<dim3(cdiv((long)S * S, 256), B), 256, 0, st>>>(box, out, S, a);
    return check_launch("g2s_prior_ellipsoid");
}
