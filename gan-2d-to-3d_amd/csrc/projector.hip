// projector.hip — what the latent projector (gan-2d-to-3d_amd/projector.py; stylegan2-pytorch/projector.py:16-44)
// adds to the frozen generator: the gradient of a noise map, and the noise regulariser / re-normalisation of ALL
// noise maps of a generator in a fixed number of launches (include/g2s.h).
//
//   g2s_noise_grad        gnoise[b,i] = noise_w * sum_c gpre[b,c,i]: one pass over the pre-activation gradient that
//                         g2s_synth_bwd_rows writes.  A workgroup owns a strip of pixels; its 256 lanes are
//                         (pixel lanes) x (channel slices); a slice adds its channels in ascending order, the slices
//                         meet in LDS and are added in ascending order: no atomics, one fixed order.
//   g2s_noise_regularize  per map n_0 [B,1,S,S]: levels n_{l+1} = 2x2 mean of n_l down to the first side <= 8; each
//                         level adds mean(n_l roll_x n_l)^2 + mean(n_l roll_y n_l)^2 (means over B S_l^2, wrapping).
//                         ONE scheme for every side 4 .. 512: the pooled levels live in the caller's workspace.
//                           launch 1  pool: a workgroup pools one tile (<= 64 x 64 of level 0) down all its levels in LDS
//                           launch 2  products: per (map, level, chunk of 4096 elements) the two partial sums
//                           launch 3  gradient: every workgroup adds the partial sums of its map in ascending chunk
//                                     order (so all agree on the means), then writes
//                                     grad = sum_l 4^-l [ (2 m_x / N_l)(n_l(x+1) + n_l(x-1)) + the same in y ](y >> l, x >> l);
//                                     the last workgroup adds the loss over maps and levels in the reference's order.
//   g2s_noise_normalize   n <- (n - mean) / std (unbiased), in place.  launch 1: (mean, M2) of every 4096-element
//                         chunk, two-pass inside the chunk; launch 2: every workgroup merges the chunk statistics of its
//                         map in ascending order (Chan's update, double) and rescales its chunk.
// None of the sums depends on g2s_set_deterministic: there is one partition, and it has a fixed order.
#include "g2s_common.h"
#include "wave_sum.h"

namespace g2s {

constexpr int NZ_THREADS = 256;
constexpr int NZ_CHUNK = 4096;           // elements per workgroup of the product / statistics passes
constexpr int NZ_TILE = 64;              // level-0 side of a pooling tile: 64 >> 6 = 1, the deepest level of side 512
constexpr int NZ_MAX_LEVELS = 7;         // 512, 256, 128, 64, 32, 16, 8

// sum over the workgroup, the same value in every thread; `red` holds 4 floats
__device__ __forceinline__ float nz_block_sum(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();                      // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------------- noise gradient
template <int V> struct nz_vec;
template <> struct nz_vec<4> { typedef float4 type; };
template <> struct nz_vec<1> { typedef float type; };
__device__ __forceinline__ void nz_add(float4 &a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void nz_add(float &a, const float b) { a += b; }
__device__ __forceinline__ float4 nz_mul(const float4 a, float s) { return float4{a.x * s, a.y * s, a.z * s, a.w * s}; }
__device__ __forceinline__ float nz_mul(const float a, float s) { return a * s; }

// grid (ceil(n / (LANES * V)), B); lane = threadIdx % LANES owns V consecutive pixels, slice = threadIdx / LANES
// owns the channels slice, slice + SLICES, ...
template <int V, int LANES>
__global__ __launch_bounds__(NZ_THREADS) void noise_grad(const float *__restrict__ gpre, const float *__restrict__ noise_w,
                                                         float *__restrict__ gnoise, int C, int n) {
    typedef typename nz_vec<V>::type vec;
    constexpr int SLICES = NZ_THREADS / LANES;
    __shared__ vec part[SLICES][LANES];
    const int lane = threadIdx.x % LANES, slice = threadIdx.x / LANES, b = blockIdx.y;
    const int i = (blockIdx.x * LANES + lane) * V;
    vec acc{};
    if (i < n) {                          // n % V == 0 on the vector path: a lane is whole or empty
        const float *p = gpre + (size_t)b * C * n + i;
#pragma unroll 4
        for (int c = slice; c < C; c += SLICES) nz_add(acc, *reinterpret_cast<const vec *>(p + (size_t)c * n));
    }
    part[slice][lane] = acc;
    __syncthreads();
    if (slice == 0 && i < n) {
        vec s = part[0][lane];
        for (int k = 1; k < SLICES; k++) nz_add(s, part[k][lane]);
        *reinterpret_cast<vec *>(gnoise + (size_t)b * n + i) = nz_mul(s, noise_w[0]);
    }
}

// ------------------------------------------------------------------------------------------------- the table of maps
struct NoiseMaps {
    float *noise[G2S_NOISE_MAX_MAPS];        // level 0 (normalize writes it)
    float *grad[G2S_NOISE_MAX_MAPS];
    int side[G2S_NOISE_MAX_MAPS], levels[G2S_NOISE_MAX_MAPS];
    int pool_off[G2S_NOISE_MAX_MAPS];        // floats into ws: levels 1 .. of this map, back to back, [B, S_l, S_l] each
    int part_off[G2S_NOISE_MAX_MAPS];        // floats into ws: 2 per (level, chunk), levels back to back
    int blk_pool[G2S_NOISE_MAX_MAPS + 1], blk_prod[G2S_NOISE_MAX_MAPS + 1], blk_grad[G2S_NOISE_MAX_MAPS + 1];
    int maps, B;
    float *ws, *loss;
};

__host__ __device__ inline int nz_levels(int side) {
    int l = 1;
    while (side > 8) { side >>= 1; l++; }
    return l;
}
__host__ __device__ inline int nz_chunks(int B, int side) { return (B * side * side + NZ_CHUNK - 1) / NZ_CHUNK; }

__device__ __forceinline__ int nz_find(const int *prefix, int maps, int blk) {
    int m = 0;
    while (m + 1 < maps && prefix[m + 1] <= blk) m++;
    return m;
}

// level l of map m: the map itself, or its pooled copy in the workspace
__device__ __forceinline__ const float *nz_level(const NoiseMaps &t, int m, int l) {
    if (l == 0) return t.noise[m];
    int off = t.pool_off[m];
    for (int j = 1; j < l; j++) off += t.B * (t.side[m] >> j) * (t.side[m] >> j);
    return t.ws + off;
}

// ------------------------------------------------------------------------------------------------- launch 1: pooling
// one workgroup per (map with > 1 level, sample, tile): the tile's whole pyramid in LDS, every level stored to ws
__global__ __launch_bounds__(NZ_THREADS) void noise_pool(NoiseMaps t) {
    __shared__ float lv[NZ_TILE * NZ_TILE + NZ_TILE * NZ_TILE / 2];     // level 0, then levels 1.. back to back
    const int m = nz_find(t.blk_pool, t.maps, blockIdx.x);
    const int S = t.side[m], L = t.levels[m];
    const int T = S < NZ_TILE ? S : NZ_TILE, tiles = S / T;
    int r = blockIdx.x - t.blk_pool[m];
    const int tx = r % tiles, ty = (r / tiles) % tiles, b = r / (tiles * tiles);
    const float *src = t.noise[m] + ((size_t)b * S + ty * T) * S + tx * T;
    for (int i = threadIdx.x; i < T * T; i += NZ_THREADS) lv[i] = src[(size_t)(i / T) * S + i % T];
    __syncthreads();
    float *cur = lv, *ws = t.ws + t.pool_off[m];
    for (int l = 1; l < L; l++) {
        const int Tc = T >> (l - 1), Tn = Tc >> 1, Sl = S >> l;      // this tile at levels l - 1 and l; map side at l
        float *nxt = cur + Tc * Tc;
        float *dst = ws + ((size_t)b * Sl + ty * Tn) * Sl + tx * Tn;
        for (int i = threadIdx.x; i < Tn * Tn; i += NZ_THREADS) {
            const int y = i / Tn, x = i % Tn;
            const float *q = cur + (2 * y) * Tc + 2 * x;
            const float v = ((q[0] + q[1]) + (q[Tc] + q[Tc + 1])) * 0.25f;
            nxt[i] = v;
            dst[(size_t)y * Sl + x] = v;
        }
        __syncthreads();
        cur = nxt;
        ws += t.B * Sl * Sl;
    }
}

// ------------------------------------------------------------------------------------------------- launch 2: products
// one workgroup per (map, level, chunk): sum n(y, x) n(y, x - 1) and sum n(y, x) n(y - 1, x) over the chunk
__global__ __launch_bounds__(NZ_THREADS) void noise_products(NoiseMaps t) {
    __shared__ float red[4];
    const int m = nz_find(t.blk_prod, t.maps, blockIdx.x);
    int r = blockIdx.x - t.blk_prod[m], l = 0, pair = 0;
    while (r >= nz_chunks(t.B, t.side[m] >> l)) {
        r -= nz_chunks(t.B, t.side[m] >> l);
        pair += nz_chunks(t.B, t.side[m] >> l);
        l++;
    }
    const int S = t.side[m] >> l, N = t.B * S * S;
    const float *n = nz_level(t, m, l);
    float sx = 0.0f, sy = 0.0f;
    for (int i = r * NZ_CHUNK + threadIdx.x; i < min(N, (r + 1) * NZ_CHUNK); i += NZ_THREADS) {
        const int x = i % S, y = (i / S) % S, base = i - y * S - x;     // base: start of the sample
        const float v = n[i];
        sx += v * n[base + y * S + ((x + S - 1) & (S - 1))];
        sy += v * n[base + ((y + S - 1) & (S - 1)) * S + x];
    }
    sx = nz_block_sum(sx, red);
    sy = nz_block_sum(sy, red);
    if (threadIdx.x == 0) {
        float *p = t.ws + t.part_off[m] + 2 * (pair + r);
        p[0] = sx;
        p[1] = sy;
    }
}

// The means of map m from the partial sums: thread (2 l + dir) * 16 + j adds the chunks j, j + 16, ... of (level l,
// direction dir) in ascending order; the 16 meet in a butterfly.  mean[2 l + dir], valid after the barrier.
__device__ __forceinline__ void nz_means(const NoiseMaps &t, int m, float *mean) {
    const int pairs = 2 * t.levels[m], pr = threadIdx.x >> 4, j = threadIdx.x & 15;
    float acc = 0.0f;
    int N = 1;
    if (pr < pairs) {
        const int l = pr >> 1;
        int first = 0;
        for (int k = 0; k < l; k++) first += nz_chunks(t.B, t.side[m] >> k);
        const int S = t.side[m] >> l, chunks = nz_chunks(t.B, S);
        N = t.B * S * S;
        const float *p = t.ws + t.part_off[m] + 2 * first + (pr & 1);
        for (int c = j; c < chunks; c += 16) acc += p[2 * c];
    }
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (pr < pairs && j == 0) mean[pr] = acc / (float)N;
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------- launch 3: gradient, loss
// workgroups of map m: 1024 elements each, 4 consecutive x per thread; one more workgroup (the last) for the loss
__global__ __launch_bounds__(NZ_THREADS) void noise_reg_grad(NoiseMaps t, int with_grad) {
    __shared__ float mean[2 * NZ_MAX_LEVELS];
    const int last = with_grad ? t.blk_grad[t.maps] : 0;
    if ((int)blockIdx.x == last) {                    // the loss: ((loss + m_x^2) + m_y^2) map by map, level by level
        float loss = 0.0f;
        for (int m = 0; m < t.maps; m++) {
            nz_means(t, m, mean);
            if (threadIdx.x == 0)
                for (int k = 0; k < 2 * t.levels[m]; k++) loss += mean[k] * mean[k];
            __syncthreads();
        }
        if (threadIdx.x == 0 && t.loss) t.loss[0] = loss;
        return;
    }
    const int m = nz_find(t.blk_grad, t.maps, blockIdx.x);
    nz_means(t, m, mean);
    const int S0 = t.side[m], L = t.levels[m], N0 = t.B * S0 * S0;
    const int i0 = ((blockIdx.x - t.blk_grad[m]) * NZ_THREADS + threadIdx.x) * 4;
    if (i0 >= N0) return;
    const int x0 = i0 % S0, y0 = (i0 / S0) % S0, b = i0 / (S0 * S0);
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float w = 1.0f;                                   // 4^-l
    for (int l = 0; l < L; l++, w *= 0.25f) {
        const int S = S0 >> l, y = y0 >> l;
        const float *n = nz_level(t, m, l) + (size_t)b * S * S;
        const float cx = w * 2.0f * mean[2 * l] / (float)(t.B * S * S), cy = w * 2.0f * mean[2 * l + 1] / (float)(t.B * S * S);
        const float *up = n + ((y + S - 1) & (S - 1)) * S, *dn = n + ((y + 1) & (S - 1)) * S, *row = n + y * S;
        float prev = 0.0f;
        int xp = -1;
        for (int k = 0; k < 4; k++) {                 // 4, 2, 1, 1, ... distinct pixels of level l under these 4
            const int x = (x0 + k) >> l;
            if (x != xp) {
                prev = cx * (row[(x + 1) & (S - 1)] + row[(x + S - 1) & (S - 1)]) + cy * (dn[x] + up[x]);
                xp = x;
            }
            g[k] += prev;
        }
    }
    *reinterpret_cast<float4 *>(t.grad[m] + i0) = float4{g[0], g[1], g[2], g[3]};
}

// ------------------------------------------------------------------------------------------------- normalisation
struct NormMaps {
    float *noise[G2S_NOISE_MAX_MAPS];
    int count[G2S_NOISE_MAX_MAPS];           // B S^2
    int blk[G2S_NOISE_MAX_MAPS + 1];         // chunk prefix; the statistics of chunk k are ws[2 k], ws[2 k + 1]
    int maps;
    float *ws;
};

__global__ __launch_bounds__(NZ_THREADS) void noise_chunk_stats(NormMaps t) {
    __shared__ float red[4];
    const int m = nz_find(t.blk, t.maps, blockIdx.x);
    const int lo = (blockIdx.x - t.blk[m]) * NZ_CHUNK, hi = min(t.count[m], lo + NZ_CHUNK);
    const float *n = t.noise[m];
    float v[NZ_CHUNK / NZ_THREADS], s = 0.0f;
#pragma unroll
    for (int k = 0; k < NZ_CHUNK / NZ_THREADS; k++) {
        const int i = lo + k * NZ_THREADS + threadIdx.x;
        v[k] = i < hi ? n[i] : 0.0f;
        s += v[k];
    }
    const float mean = nz_block_sum(s, red) / (float)(hi - lo);
    float q = 0.0f;
#pragma unroll
    for (int k = 0; k < NZ_CHUNK / NZ_THREADS; k++) {
        const int i = lo + k * NZ_THREADS + threadIdx.x;
        const float d = i < hi ? v[k] - mean : 0.0f;
        q += d * d;
    }
    q = nz_block_sum(q, red);
    if (threadIdx.x == 0) {
        t.ws[2 * blockIdx.x] = mean;
        t.ws[2 * blockIdx.x + 1] = q;
    }
}

__global__ __launch_bounds__(NZ_THREADS) void noise_rescale(NormMaps t) {
    __shared__ float stat[2];
    const int m = nz_find(t.blk, t.maps, blockIdx.x);
    const int lo = (blockIdx.x - t.blk[m]) * NZ_CHUNK, hi = min(t.count[m], lo + NZ_CHUNK);
    if (threadIdx.x == 0) {                   // merge the chunks of this map in ascending order
        double mean = 0.0, m2 = 0.0, cnt = 0.0;
        for (int c = t.blk[m]; c < t.blk[m + 1]; c++) {
            const double nb = (double)min(NZ_CHUNK, t.count[m] - (c - t.blk[m]) * NZ_CHUNK);
            const double d = (double)t.ws[2 * c] - mean, tot = cnt + nb;
            mean += d * nb / tot;
            m2 += (double)t.ws[2 * c + 1] + d * d * cnt * nb / tot;
            cnt = tot;
        }
        stat[0] = (float)mean;
        stat[1] = (float)sqrt(m2 / (cnt - 1.0));
    }
    __syncthreads();
    const float mean = stat[0], sd = stat[1];
    float *n = t.noise[m];
    for (int i = lo + threadIdx.x; i < hi; i += NZ_THREADS) n[i] = (n[i] - mean) / sd;
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_noise_grad(const float *gpre, const float *noise_w, float *gnoise, int B, int C, int n,
                              g2s_stream_t stream) {
    G2S_REQUIRE(gpre && noise_w && gnoise, "g2s_noise_grad: NULL pointer argument");
    G2S_REQUIRE(B > 0 && B <= 65535 && C > 0 && n > 0, "g2s_noise_grad: 1 <= B <= 65535, C and n positive");
    const bool vec = n % 4 == 0 && (((uintptr_t)gpre | (uintptr_t)gnoise) & 15) == 0;
    if (vec) noise_grad<4, 16><<<dim3(cdiv(n, 64), B), NZ_THREADS, 0, as_stream(stream)>>>(gpre, noise_w, gnoise, C, n);
    else noise_grad<1, 64><<<dim3(cdiv(n, 64), B), NZ_THREADS, 0, as_stream(stream)>>>(gpre, noise_w, gnoise, C, n);
    return check_launch("g2s_noise_grad");
}

static int noise_check_sides(const char *who, const int *sides, int maps, int B) {
    G2S_REQUIRE(sides, "%s: NULL sides", who);
    G2S_REQUIRE(maps > 0 && maps <= G2S_NOISE_MAX_MAPS, "%s: 1 <= maps <= %d", who, G2S_NOISE_MAX_MAPS);
    G2S_REQUIRE(B > 0 && B <= 64, "%s: 1 <= B <= 64", who);
    for (int m = 0; m < maps; m++)
        G2S_REQUIRE(sides[m] >= 4 && sides[m] <= 512 && (sides[m] & (sides[m] - 1)) == 0,
                    "%s: map %d: the side must be a power of two, 4 .. 512 (got %d)", who, m, sides[m]);
    return G2S_OK;
}

// offsets and workgroup prefixes of the regulariser; returns the workspace floats
static size_t noise_reg_layout(NoiseMaps &t, const int *sides, int maps, int B) {
    size_t off = 0;
    t.maps = maps;
    t.B = B;
    t.blk_pool[0] = t.blk_prod[0] = t.blk_grad[0] = 0;
    for (int m = 0; m < maps; m++) {
        const int S = sides[m], L = nz_levels(S);
        t.side[m] = S;
        t.levels[m] = L;
        t.pool_off[m] = (int)off;
        for (int l = 1; l < L; l++) off += (size_t)B * (S >> l) * (S >> l);
        const int T = S < NZ_TILE ? S : NZ_TILE;
        t.blk_pool[m + 1] = t.blk_pool[m] + (L > 1 ? B * (S / T) * (S / T) : 0);
        int chunks = 0;
        for (int l = 0; l < L; l++) chunks += nz_chunks(B, S >> l);
        t.blk_prod[m + 1] = t.blk_prod[m] + chunks;
        t.blk_grad[m + 1] = t.blk_grad[m] + cdiv((long)B * S * S, NZ_THREADS * 4);
    }
    for (int m = 0; m < maps; m++) {
        t.part_off[m] = (int)off;
        off += 2 * (size_t)(t.blk_prod[m + 1] - t.blk_prod[m]);
    }
    return off;
}

extern "C" size_t g2s_noise_regularize_workspace_bytes(const int *sides, int maps, int B) {
    if (noise_check_sides("g2s_noise_regularize_workspace_bytes", sides, maps, B) != G2S_OK) return 0;
    NoiseMaps t{};
    return noise_reg_layout(t, sides, maps, B) * sizeof(float);
}

extern "C" int g2s_noise_regularize(const void *const *noise, const void *const *grad, const int *sides, int maps, int B,
                                    float *loss, void *workspace, size_t workspace_bytes, g2s_stream_t stream) {
    G2S_REQUIRE(noise && loss, "g2s_noise_regularize: NULL pointer argument");
    const int rc = noise_check_sides("g2s_noise_regularize", sides, maps, B);
    if (rc != G2S_OK) return rc;
    NoiseMaps t{};
    const size_t need = noise_reg_layout(t, sides, maps, B) * sizeof(float);
    for (int m = 0; m < maps; m++) {
        G2S_REQUIRE(noise[m] && (!grad || grad[m]), "g2s_noise_regularize: map %d: NULL pointer", m);
        G2S_REQUIRE(!grad || ((uintptr_t)grad[m] & 15) == 0, "g2s_noise_regularize: map %d: grad must be 16-byte aligned", m);
        t.noise[m] = (float *)noise[m];
        t.grad[m] = grad ? (float *)grad[m] : nullptr;
    }
    if (!workspace || workspace_bytes < need)
        return fail(G2S_ERR_WORKSPACE, "g2s_noise_regularize: workspace of %zu bytes, %zu needed",
                    workspace ? workspace_bytes : (size_t)0, need);
    G2S_REQUIRE(((uintptr_t)workspace & 3) == 0, "g2s_noise_regularize: workspace must be 4-byte aligned");
    t.ws = (float *)workspace;
    t.loss = loss;
    hipStream_t st = as_stream(stream);
    if (t.blk_pool[maps] > 0) noise_pool<<<t.blk_pool[maps], NZ_THREADS, 0, st>>>(t);
    noise_products<<<t.blk_prod[maps], NZ_THREADS, 0, st>>>(t);
    noise_reg_grad<<<(grad ? t.blk_grad[maps] : 0) + 1, NZ_THREADS, 0, st>>>(t, grad ? 1 : 0);
    return check_launch("g2s_noise_regularize");
}

static int noise_norm_layout(NormMaps &t, const int *sides, int maps, int B) {
    t.maps = maps;
    t.blk[0] = 0;
    for (int m = 0; m < maps; m++) {
        t.count[m] = B * sides[m] * sides[m];
        t.blk[m + 1] = t.blk[m] + nz_chunks(B, sides[m]);
    }
    return t.blk[maps];
}

extern "C" size_t g2s_noise_normalize_workspace_bytes(const int *sides, int maps, int B) {
    if (noise_check_sides("g2s_noise_normalize_workspace_bytes", sides, maps, B) != G2S_OK) return 0;
    NormMaps t{};
    return (size_t)noise_norm_layout(t, sides, maps, B) * 2 * sizeof(float);
}

extern "C" int g2s_noise_normalize(const void *const *noise, const int *sides, int maps, int B, void *workspace,
                                   size_t workspace_bytes, g2s_stream_t stream) {
    G2S_REQUIRE(noise, "g2s_noise_normalize: NULL pointer argument");
    const int rc = noise_check_sides("g2s_noise_normalize", sides, maps, B);
    if (rc != G2S_OK) return rc;
    NormMaps t{};
    const int chunks = noise_norm_layout(t, sides, maps, B);
    const size_t need = (size_t)chunks * 2 * sizeof(float);
    for (int m = 0; m < maps; m++) {
        G2S_REQUIRE(noise[m], "g2s_noise_normalize: map %d: NULL pointer", m);
        t.noise[m] = (float *)noise[m];
    }
    if (!workspace || workspace_bytes < need)
        return fail(G2S_ERR_WORKSPACE, "g2s_noise_normalize: workspace of %zu bytes, %zu needed",
                    workspace ? workspace_bytes : (size_t)0, need);
    G2S_REQUIRE(((uintptr_t)workspace & 3) == 0, "g2s_noise_normalize: workspace must be 4-byte aligned");
    t.ws = (float *)workspace;
    hipStream_t st = as_stream(stream);
    noise_chunk_stats<<<chunks, NZ_THREADS, 0, st>>>(t);
    noise_rescale<<<chunks, NZ_THREADS, 0, st>>>(t);
    return check_launch("g2s_noise_normalize");
}
