// resample.hip — a separable banded resampler: the linear map  y = Ay · x · Axᵀ  per plane, where every row of Ay and
// of Ax is one contiguous band of taps (op/resample.py builds the bands of step 2's centre crop
//
//   resize(x, origin) -> centre crop -> resize(., image)          (GAN2Shape/model.py:197-200, 211-214)
//
// and of its transpose, so the forward, the backward and every higher derivative of that chain are this one kernel
// with two small tables).
//
//   y[p, i, j] = sum_{a < ylen[i]} yw[i Ky + a] * ( sum_{b < xlen[j]} xw[j Kx + b] * x[p, ylo[i] + a, xlo[j] + b] )
//
// One workgroup = one plane x one tile of TR output rows:
//   1. the input rows the tile's bands touch, restricted to the columns any band touches, go into LDS (a wave per row,
//      lanes along the row: coalesced; the cropped-away border is never read);
//   2. the horizontal pass runs out of LDS into LDS (a lane per output column, its taps in registers);
//   3. the vertical pass runs out of LDS into coalesced stores.
// Each sum is an ascending fmaf chain from 0, every output element is written by exactly one thread, there are no
// atomics: two calls are bit-identical.  An empty band (len 0) writes 0 — the backward of a crop relies on it.
//
// The tables are device memory, so the launcher cannot read them: g2s_resample_bands_check (host tables, called once
// when a table is made) is where a band that leaves the input is refused.  The kernel, for its part, clamps what it
// stages to the input and to its LDS and skips a tap outside what it staged, so a table that never went through the
// check gives wrong numbers, not a wild read.
#include "g2s_common.h"

namespace g2s {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_TAPS = 8;          // cap of Ky and Kx (the crop chains need 2-5)
constexpr int RS_MAX_TILE = 12;         // output rows per workgroup, at most
constexpr int RS_LDS_BYTES = 64 * 1024;
constexpr int RS_HEAD = 4;              // ints in front of the LDS image: the column range (lo, hi)

// LDS floats of a tile of `tr` output rows: the header, the staged band [rows][cols] and its horizontal pass
// [rows][Wout].  Consecutive bands overlap or abut (g2s_resample_bands_check), so a tile touches at most tr * Ky rows
// and the whole output at most Wout * Kx columns.
inline long rs_rows_cap(int tr, int Ky, int Hin) { return (long)tr * Ky < Hin ? (long)tr * Ky : Hin; }
inline long rs_cols_cap(int Wout, int Kx, int Win) { return (long)Wout * Kx < Win ? (long)Wout * Kx : Win; }
inline long rs_lds_floats(int tr, int Ky, int Kx, int Hin, int Win, int Wout) {
    return RS_HEAD + rs_rows_cap(tr, Ky, Hin) * (rs_cols_cap(Wout, Kx, Win) + Wout);
}

// grid (tiles * planes); dynamic LDS = rs_lds_floats(TR, ...) floats
__global__ __launch_bounds__(RS_THREADS) void resample_sep_kernel(
        const float *__restrict__ x, float *__restrict__ y, int Hin, int Win, int Hout, int Wout,
        const int *__restrict__ ylo, const int *__restrict__ ylen, const float *__restrict__ yw, int Ky,
        const int *__restrict__ xlo, const int *__restrict__ xlen, const float *__restrict__ xw, int Kx,
        int TR, int tiles, int rows_cap, int cols_cap) {
    extern __shared__ float lds[];
    int *head = reinterpret_cast<int *>(lds);
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles;
    const size_t p = blockIdx.x / tiles;
    const int i0 = tile * TR, i1 = min(i0 + TR, Hout);

    // rows the tile reads: uniform over the workgroup
    int r0 = Hin, r1 = 0;
    for (int i = i0; i < i1; ++i) {
        const int n = min(ylen[i], Ky);
        if (n > 0) { r0 = min(r0, ylo[i]); r1 = max(r1, ylo[i] + n); }
    }
    r0 = max(r0, 0);
    r1 = min(min(r1, Hin), r0 + rows_cap);
    const int nrows = max(r1 - r0, 0);

    // columns any band reads
    if (tid == 0) { head[0] = Win; head[1] = 0; }
    __syncthreads();
    {
        int c0 = Win, c1 = 0;
        for (int j = tid; j < Wout; j += RS_THREADS) {
            const int n = min(xlen[j], Kx);
            if (n > 0) { c0 = min(c0, xlo[j]); c1 = max(c1, xlo[j] + n); }
        }
        if (c0 < c1) { atomicMin(&head[0], c0); atomicMax(&head[1], c1); }
    }
    __syncthreads();
    const int c0 = max(head[0], 0);
    const int c1 = min(min(head[1], Win), c0 + cols_cap);
    const int ncols = max(c1 - c0, 0);

    float *s_in = lds + RS_HEAD;                    // [nrows][ncols]
    float *s_h = s_in + (size_t)nrows * ncols;      // [nrows][Wout]

    // 1. stage: a wave per row, lanes along the row
    const float *xp = x + p * Hin * Win;
    for (int rr = tid >> 6; rr < nrows; rr += RS_THREADS / 64) {
        const float *src = xp + (size_t)(r0 + rr) * Win + c0;
        for (int cc = tid & 63; cc < ncols; cc += 64) s_in[rr * ncols + cc] = src[cc];
    }
    __syncthreads();

    // lanes along the output row; an output narrower than the workgroup gives the spare waves rows of their own
    const int LW = Wout <= 64 ? 64 : Wout <= 128 ? 128 : RS_THREADS;
    const int lane = tid % LW, grp = tid / LW, ngrp = RS_THREADS / LW;

    // 2. horizontal pass: a lane per output column, its taps in registers, down the staged rows
    for (int j = lane; j < Wout; j += LW) {
        const int n = ncols > 0 ? min(xlen[j], Kx) : 0, lo = xlo[j] - c0;
        float w[RS_MAX_TAPS];
#pragma unroll
        for (int b = 0; b < RS_MAX_TAPS; ++b) w[b] = (b < n && lo + b >= 0 && lo + b < ncols) ? xw[j * Kx + b] : 0.0f;
        for (int rr = grp; rr < nrows; rr += ngrp) {
            const float *row = s_in + rr * ncols;
            float acc = 0.0f;
#pragma unroll
            for (int b = 0; b < RS_MAX_TAPS; ++b)
                if (b < n) acc = fmaf(w[b], row[min(max(lo + b, 0), ncols - 1)], acc);
            s_h[rr * Wout + j] = acc;
        }
    }
    __syncthreads();

    // 3. vertical pass
    float *yp = y + p * Hout * Wout;
    for (int i = i0 + grp; i < i1; i += ngrp) {
        const int n = min(ylen[i], Ky), lo = ylo[i] - r0;
        for (int j = lane; j < Wout; j += LW) {
            float acc = 0.0f;
            for (int a = 0; a < n; ++a) {
                const int rr = lo + a;
                if (rr >= 0 && rr < nrows) acc = fmaf(yw[i * Ky + a], s_h[rr * Wout + j], acc);
            }
            yp[(size_t)i * Wout + j] = acc;
        }
    }
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_resample_max_taps(void) { return RS_MAX_TAPS; }

extern "C" int g2s_resample_tile_rows(int Hin, int Win, int Hout, int Wout, int Ky, int Kx) {
    if (Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || Ky < 1 || Kx < 1 || Ky > RS_MAX_TAPS || Kx > RS_MAX_TAPS) return 0;
    int tr = Hout < RS_MAX_TILE ? Hout : RS_MAX_TILE;
    while (tr > 0 && rs_lds_floats(tr, Ky, Kx, Hin, Win, Wout) * 4 > RS_LDS_BYTES) --tr;
    return tr;
}

extern "C" int g2s_resample_bands_check(const int *lo, const int *len, int n_out, int K, int n_in) {
    G2S_REQUIRE(lo && len, "NULL pointer argument");
    G2S_REQUIRE(n_out > 0 && n_in > 0, "bad size");
    G2S_REQUIRE(K >= 1 && K <= RS_MAX_TAPS, "K = %d taps: the kernel holds 1..%d", K, RS_MAX_TAPS);
    long prev_lo = -1, prev_hi = -1;
    for (int i = 0; i < n_out; ++i) {
        G2S_REQUIRE(len[i] >= 0 && len[i] <= K, "band %d has %d taps, the table holds %d", i, len[i], K);
        if (len[i] == 0) continue;
        const long hi = (long)lo[i] + len[i];
        G2S_REQUIRE(lo[i] >= 0 && hi <= n_in, "band %d = [%d, %ld) leaves the input [0, %d)", i, lo[i], hi, n_in);
        // what the LDS bound of a tile rests on: the bands ascend, and consecutive ones overlap or abut
        G2S_REQUIRE(prev_hi < 0 || (lo[i] >= prev_lo && hi >= prev_hi && lo[i] <= prev_hi),
                    "band %d = [%d, %ld) does not follow [%ld, %ld): bands must ascend without a gap", i, lo[i], hi,
                    prev_lo, prev_hi);
        prev_lo = lo[i];
        prev_hi = hi;
    }
    return G2S_OK;
}

extern "C" int g2s_resample_sep(const float *x, float *y, int planes, int Hin, int Win, int Hout, int Wout,
                                const int *ylo, const int *ylen, const float *yw, int Ky,
                                const int *xlo, const int *xlen, const float *xw, int Kx, g2s_stream_t stream) {
    G2S_REQUIRE(x && y && ylo && ylen && yw && xlo && xlen && xw, "NULL pointer argument");
    G2S_REQUIRE(Ky >= 1 && Ky <= RS_MAX_TAPS && Kx >= 1 && Kx <= RS_MAX_TAPS, "Ky = %d, Kx = %d taps: the kernel holds 1..%d",
                Ky, Kx, RS_MAX_TAPS);
    G2S_REQUIRE(planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "bad size");
    G2S_REQUIRE((long)Hin * Win < (1L << 30) && (long)Hout * Wout < (1L << 30), "a plane of 2^30 elements or more");
    const int tr = g2s_resample_tile_rows(Hin, Win, Hout, Wout, Ky, Kx);
    G2S_REQUIRE(tr > 0, "rows of %d -> %d columns with %d taps do not fit the %d KB of LDS", Win, Wout, Kx, RS_LDS_BYTES / 1024);
    const int tiles = cdiv(Hout, tr);
    G2S_REQUIRE((long)tiles * planes < (1L << 31), "too many planes");
    const size_t lds = (size_t)rs_lds_floats(tr, Ky, Kx, Hin, Win, Wout) * 4;
    resample_sep_kernel<<<dim3((unsigned)(tiles * planes)), RS_THREADS, lds, as_stream(stream)>>>(
        x, y, Hin, Win, Hout, Wout, ylo, ylen, yw, Ky, xlo, xlen, xw, Kx, tr, tiles,
        (int)rs_rows_cap(tr, Ky, Hin), (int)rs_cols_cap(Wout, Kx, Win));
    return check_launch("g2s_resample_sep");
}
