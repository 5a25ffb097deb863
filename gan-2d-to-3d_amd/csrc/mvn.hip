// mvn.hip — mean, covariance and block Cholesky factor of rows [N, D] in ONE launch (view_light.py mvn_fit: the fit
// of the view and light priors from a trained model's estimates; D = 10 with blocks (6, 4) there).
//
// ONE workgroup of 256 threads, one wave per SIMD.  Thread t takes rows t, t + 256, ... in ascending order:
//   pass 1  per-thread column sums in double                         -> mean (double, kept in LDS)
//   pass 2  per-thread sums of (x_i - mean_i)(x_j - mean_j), i <= j  -> cov = sum / (N - 1) (+ ridge on the diagonal)
//   then    right-looking Cholesky in double on each diagonal block of the double covariance, D columns, two barriers
//           per column, one thread per matrix entry.
// A one-pass sum of squares would cancel (rows 1000 + 0.01 z lose every digit in fp32 and nine in double), so the
// second read is the price of the centring; at the sizes of the call (N = 1e5, D = 10: 4 MB) it comes from L2.
//
// Partials meet in LDS in a fixed two-level tree of fan-in 16: the per-thread accumulators go to LDS 16 values at a
// time ([thread][16 + 1 pad] doubles: the 17-double row stride puts the 16 lanes of a ds_write_b64 group on distinct
// banks, and the two 16-thread groups of a 32-lane ds_read_b64 group 32 banks apart); thread (g, v) adds the 16
// partials of threads 16 g .. 16 g + 15 for value v in ascending order, then threads 0 .. 15 add the 16 group sums.
// No atomics, no workspace, no second launch: bit-identical from run to run.
//
// Registers: D is a template parameter, so the D (D + 1) / 2 accumulators (136 doubles at D = 16) and the 2 or 4 rows
// in flight stay in VGPRs (512 per lane at one wave per SIMD).  The double FMAs of pass 2 run at a quarter of the
// fp32 rate (55 per row at D = 10); the row loads are dwords, or 8-byte pairs when D, ld and the base allow it, and
// the rows of a trip are requested before the first is used.  The call is bound by one workgroup's latency, not by HBM
// (tools/bench_view_light.py has the figures); it is deliberately not spread over the grid, which would need a second
// launch or an in-grid hand-off.
//
// A non-finite input makes the double column sum non-finite (a finite sum of < 2^31 floats cannot overflow a double,
// inf - inf and NaN stay NaN), so status -1 is read off the sums of pass 1.
#include <cmath>
#include <cstdint>
#include "g2s_common.h"

namespace g2s {

constexpr int MV_THREADS = 256;
constexpr int MV_MAX_D = G2S_MVN_MAX_D;
// rows in flight per thread: fewer beside the 91+ accumulators of the widest D, which would otherwise spill
constexpr int mv_rows_ahead(int D) { return D > 12 ? 2 : 4; }
constexpr int MV_CH = 16;           // values per trip through the LDS tree (and its fan-in)
constexpr int MV_MAX_K = MV_MAX_D * (MV_MAX_D + 1) / 2;

static_assert(MV_THREADS == MV_CH * MV_CH && MV_MAX_D <= MV_CH, "one thread per matrix entry, fan-in 16 twice");
static_assert(G2S_MVN_MAX_BLOCKS <= 4 && MV_MAX_D <= 16, "MvnParams::blk: 2 bits per column in 32");

struct MvnParams {
    const float *rows;
    float *mean, *cov, *tril;
    int *status;
    long N, ld;
    double ridge;
    unsigned blk;                   // block number of column c in bits 2 c, 2 c + 1
};

__device__ inline int mv_blk(const MvnParams &p, int c) { return (p.blk >> (2 * c)) & 3; }

struct MvnShared {
    double part[MV_THREADS][MV_CH + 1];
    double grp[MV_CH][MV_CH + 1];
    double tot[MV_MAX_K];
    double a[MV_MAX_D][MV_MAX_D + 1];       // the covariance, then the trailing matrix of the factorisation
    double l[MV_MAX_D][MV_MAX_D + 1];
};

// acc[K] of every thread -> s.tot[K]; fixed order, all threads call it
template <int K>
__device__ inline void mv_tree(const double (&acc)[K], MvnShared &s) {
    const int t = threadIdx.x, v = t % MV_CH, g = t / MV_CH;
#pragma unroll
    for (int c0 = 0; c0 < K; c0 += MV_CH) {
#pragma unroll
        for (int c = 0; c < MV_CH; c++) s.part[t][c] = c0 + c < K ? acc[c0 + c < K ? c0 + c : 0] : 0.0;
        __syncthreads();
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < MV_CH; i++) sum += s.part[g * MV_CH + i][v];
        s.grp[g][v] = sum;
        __syncthreads();
        if (t < MV_CH && c0 + t < K) {
            double tot = 0.0;
#pragma unroll
            for (int i = 0; i < MV_CH; i++) tot += s.grp[i][t];
            s.tot[c0 + t] = tot;
        }
        // the next trip's part[] writes follow this trip's reads of it by a barrier; grp[] is rewritten only after
        // the next trip's first barrier, which the threads reading it here have then passed
    }
    __syncthreads();
}

template <int D, bool V2>
__device__ inline void mv_load(const float *row, float (&x)[D]) {
    if constexpr (V2) {
        const float2 *p = reinterpret_cast<const float2 *>(row);
#pragma unroll
        for (int c = 0; c < D / 2; c++) {
            const float2 q = p[c];
            x[2 * c] = q.x, x[2 * c + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < D; c++) x[c] = row[c];
    }
}

// calls f(x) for rows t, t + 256, ... in ascending order, mv_rows_ahead(D) rows requested at a time
template <int D, bool V2, typename F>
__device__ inline void mv_rows(const MvnParams &p, F f) {
    long r = threadIdx.x;
    const long step = MV_THREADS;
    constexpr int R = mv_rows_ahead(D);
    for (; r + (R - 1) * step < p.N; r += R * step) {
        float x[R][D];
#pragma unroll
        for (int u = 0; u < R; u++) mv_load<D, V2>(p.rows + (r + u * step) * p.ld, x[u]);
#pragma unroll
        for (int u = 0; u < R; u++) f(x[u]);
    }
    for (; r < p.N; r += step) {
        float x[D];
        mv_load<D, V2>(p.rows + r * p.ld, x);
        f(x);
    }
}

template <int D, bool V2>
__global__ __launch_bounds__(MV_THREADS) void mvn_fit_kernel(MvnParams p) {
    constexpr int K = D * (D + 1) / 2;
    __shared__ MvnShared s;
    const int t = threadIdx.x;

    {   // pass 1: column sums
        double acc[D];
#pragma unroll
        for (int c = 0; c < D; c++) acc[c] = 0.0;
        mv_rows<D, V2>(p, [&](const float (&x)[D]) {
#pragma unroll
            for (int c = 0; c < D; c++) acc[c] += (double)x[c];
        });
        mv_tree<D>(acc, s);
    }
    bool finite = true;
    double mean[D];
#pragma unroll
    for (int c = 0; c < D; c++) {
        finite = finite && std::isfinite(s.tot[c]);
        mean[c] = s.tot[c] / (double)p.N;
    }
    if (t < D) p.mean[t] = (float)(s.tot[t] / (double)p.N);
    __syncthreads();                                        // tot[] is rewritten by pass 2

    {   // pass 2: centred products, upper triangle, row-major (i, j >= i)
        double acc[K];
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] = 0.0;
        mv_rows<D, V2>(p, [&](const float (&x)[D]) {
            double d[D];
#pragma unroll
            for (int c = 0; c < D; c++) d[c] = (double)x[c] - mean[c];
            int k = 0;
#pragma unroll
            for (int i = 0; i < D; i++)
#pragma unroll
                for (int j = i; j < D; j++) acc[k++] += d[i] * d[j];
        });
        mv_tree<K>(acc, s);
    }

    // one thread per entry (i, j) of the matrices
    const int i = t / MV_CH, j = t % MV_CH;
    const bool in = i < D && j < D;
    const bool low = in && j <= i && mv_blk(p, i) == mv_blk(p, j);        // inside a diagonal block, lower
    if (in) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        double c = s.tot[lo * D - lo * (lo - 1) / 2 + (hi - lo)] / (double)(p.N - 1);
        if (i == j) c += p.ridge;
        p.cov[i * D + j] = (float)c;        // (i, j) and (j, i) round the same double: exactly symmetric
        s.a[i][j] = c;
        s.l[i][j] = 0.0;
    }
    int status = finite ? 0 : -1;
    if (finite) {
        for (int c = 0; c < D; c++) {       // uniform: every thread reads the same pivot
            __syncthreads();
            const double piv = s.a[c][c];
            if (!(piv > 0.0)) {             // NaN included
                status = 1 + c;
                break;
            }
            const double root = sqrt(piv);
            if (low && j == c) s.l[i][c] = i == c ? root : s.a[i][c] / root;
            __syncthreads();
            if (low && j > c && mv_blk(p, c) == mv_blk(p, i)) s.a[i][j] -= s.l[i][c] * s.l[j][c];
        }
    }
    __syncthreads();
    if (in) p.tril[i * D + j] = low ? (float)s.l[i][j] : 0.0f;
    if (t == 0) *p.status = status;
}

template <int D>
static void mv_launch(const MvnParams &p, bool v2, hipStream_t stream) {
    if constexpr (D % 2 == 0) {
        if (v2) {
            mvn_fit_kernel<D, true><<<1, MV_THREADS, 0, stream>>>(p);
            return;
        }
    }
    mvn_fit_kernel<D, false><<<1, MV_THREADS, 0, stream>>>(p);
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_mvn_fit(const float *rows, long N, int D, long ld, const int *blocks, int nblk, double ridge,
                           float *mean, float *cov, float *tril, int *status, g2s_stream_t stream) {
    const char *what = "g2s_mvn_fit";
    G2S_REQUIRE(rows && blocks && mean && cov && tril && status, "%s: NULL pointer", what);
    G2S_REQUIRE(D >= 1 && D <= MV_MAX_D, "%s: D must be 1 .. %d, got %d", what, MV_MAX_D, D);
    G2S_REQUIRE(N >= 2 && N < (1l << 31), "%s: N must be 2 .. 2^31 - 1, got %ld", what, N);
    G2S_REQUIRE(ld >= D && ld < (1l << 31), "%s: the row stride %ld is below D = %d or too large", what, ld, D);
    G2S_REQUIRE(nblk >= 1 && nblk <= G2S_MVN_MAX_BLOCKS, "%s: 1 .. %d blocks, got %d", what, G2S_MVN_MAX_BLOCKS, nblk);
    G2S_REQUIRE(std::isfinite(ridge) && ridge >= 0.0, "%s: ridge must be finite and >= 0", what);
    MvnParams p;
    p.blk = 0;
    int col = 0;
    for (int b = 0; b < nblk; b++) {
        G2S_REQUIRE(blocks[b] >= 1 && blocks[b] <= D - col, "%s: the blocks must be positive and sum to D = %d", what, D);
        for (int c = 0; c < blocks[b]; c++) p.blk |= (unsigned)b << (2 * col++);
    }
    G2S_REQUIRE(col == D, "%s: the blocks sum to %d, not to D = %d", what, col, D);
    p.rows = rows, p.mean = mean, p.cov = cov, p.tril = tril, p.status = status;
    p.N = N, p.ld = ld, p.ridge = ridge;
    const bool v2 = D % 2 == 0 && ld % 2 == 0 && (uintptr_t)rows % 8 == 0;
    hipStream_t st = as_stream(stream);
    switch (D) {
#define MV_CASE(d) case d: mv_launch<d>(p, v2, st); break;
        MV_CASE(1) MV_CASE(2) MV_CASE(3) MV_CASE(4) MV_CASE(5) MV_CASE(6) MV_CASE(7) MV_CASE(8)
        MV_CASE(9) MV_CASE(10) MV_CASE(11) MV_CASE(12) MV_CASE(13) MV_CASE(14) MV_CASE(15) MV_CASE(16)
#undef MV_CASE
    }
    return check_launch(what);
}
