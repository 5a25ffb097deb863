// bank.hip — the gather of the projected-sample bank (bank.py SampleBank.gather; step 3 of the trainers with
// collect_iters on): ONE launch builds both hand-off tensors of a step-3 iteration from rows picked by a DEVICE index,
//   out_img  [h + b, 3, S, S]: rows 0 .. h are `head` (the input image; h is 0 or 1 in the trainers), row h + j is
//                              bank_img[idx[j]]
//   out_mask [b, 1, S, S]:     row j is bank_mask[idx[j]]
// so the torch.cat([images, projected_samples]) that opens step 3 has nothing left to do.
//
// Grid: blockIdx.x is an output row (h head rows, b image rows, b mask rows), blockIdx.y a chunk of that row.  The index
// is therefore read once per workgroup, as a uniform load, and no thread divides.  A thread moves BG_PER_THREAD units
// (float4 or float) whose loads are all issued before the first store.  At the sizes of the workload (b = 8, S = 128:
// 2.3 MB read and as much written) the launch is latency-bound, not bandwidth-bound, so the grid aims at having every
// byte in flight at once on fewer workgroups than there are CUs.  gridDim.y is sized from the image rows: 17 rows x
// 12 chunks = 204 workgroups are launched; the 9 image rows fill all 12 chunks (108 workgroups with four independent
// 16-byte loads in flight per lane), a mask row is a third as long and fills 4 (32 workgroups), and the other 8 chunks
// of each mask row (64 workgroups) find nothing to do and exit at once.  140 workgroups carry the copy.  This shape
// was chosen by that reasoning and not by a sweep: the measured call (tools/bench_sample_bank.py) sits at the floor of
// an eager launch at both sizes, which shows host pacing and does not discriminate between grids.  Plain vector
// stores: the outputs are read next by the same stream's kernels, from the L2 they were written to.
//
// A unit is a float4 when the row length is a multiple of 4 floats and every base address of that copy is 16-byte
// aligned (rows then start on 16-byte boundaries), a float otherwise (odd S, or views at an offset); the choice is made
// per copy (image rows with the head / mask rows).  No atomics, no LDS.
//
// An index outside 0 .. rows - 1 is clamped, so nothing is read out of bounds, and the position of one such entry
// (j + 1) is stored to *err with a plain store by one lane (several bad entries race benignly: any one of them is
// reported).  The host reads the word at its next call (bank.py).
#include "g2s_common.h"

namespace g2s {

constexpr int BG_THREADS = 256;
constexpr int BG_PER_THREAD = 4;
constexpr int BG_MAX_CHUNKS = 1024;     // gridDim.y; longer rows stride over it

typedef float bg_v4 __attribute__((ext_vector_type(4)));

struct BankGatherParams {
    const float *bank_img, *bank_mask, *head;
    float *out_img, *out_mask;
    const void *idx;
    int *err;
    long row_img, row_mask;     // floats per row: 3 S S, S S
    long rows;                  // rows of the bank
    int b, h, idx64, vec_img, vec_mask;
};

template <typename T>
__device__ inline void bg_copy(const float *src, float *dst, long units, int chunk, int chunks) {
    const T *s = reinterpret_cast<const T *>(src);
    T *d = reinterpret_cast<T *>(dst);
    const long span = (long)BG_THREADS * BG_PER_THREAD;
    for (long base = (long)chunk * span; base < units; base += (long)chunks * span) {
        T v[BG_PER_THREAD];
#pragma unroll
        for (int k = 0; k < BG_PER_THREAD; k++) {
            const long u = base + k * BG_THREADS + threadIdx.x;
            if (u < units) v[k] = s[u];
        }
#pragma unroll
        for (int k = 0; k < BG_PER_THREAD; k++) {
            const long u = base + k * BG_THREADS + threadIdx.x;
            if (u < units) d[u] = v[k];
        }
    }
}

__global__ __launch_bounds__(BG_THREADS) void bank_gather_kernel(BankGatherParams p) {
    const int r = blockIdx.x;           // 0 .. h + 2 b - 1
    const float *src;
    float *dst;
    long len;
    int vec;
    if (r < p.h) {
        src = p.head + (long)r * p.row_img, dst = p.out_img + (long)r * p.row_img, len = p.row_img, vec = p.vec_img;
    } else {
        const bool is_mask = r >= p.h + p.b;
        const int j = is_mask ? r - p.h - p.b : r - p.h;
        long i = p.idx64 ? (long)reinterpret_cast<const long long *>(p.idx)[j]
                         : (long)reinterpret_cast<const int *>(p.idx)[j];
        if (i < 0 || i >= p.rows) {
            if (blockIdx.y == 0 && threadIdx.x == 0) *p.err = j + 1;
            i = i < 0 ? 0 : p.rows - 1;
        }
        if (is_mask) {
            src = p.bank_mask + i * p.row_mask, dst = p.out_mask + (long)j * p.row_mask, len = p.row_mask, vec = p.vec_mask;
        } else {
            src = p.bank_img + i * p.row_img, dst = p.out_img + (long)(p.h + j) * p.row_img, len = p.row_img, vec = p.vec_img;
        }
    }
    if (vec) bg_copy<bg_v4>(src, dst, len / 4, blockIdx.y, gridDim.y);
    else bg_copy<float>(src, dst, len, blockIdx.y, gridDim.y);
}

static bool bg_aligned(const void *a, const void *b, const void *c) {
    return ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16 == 0;      // NULL (an absent head) is aligned
}

}  // namespace g2s

using namespace g2s;

extern "C" int g2s_bank_gather(const float *bank_img, const float *bank_mask, long rows, const void *idx, int idx64,
                               int b, const float *head, int h, float *out_img, float *out_mask, int S, int *err,
                               g2s_stream_t stream) {
    const char *what = "g2s_bank_gather";
    G2S_REQUIRE(bank_img && bank_mask && idx && out_img && out_mask && err, "%s: NULL pointer", what);
    G2S_REQUIRE(rows > 0 && b > 0 && S > 0 && h >= 0, "%s: rows, b, S must be positive and h >= 0", what);
    G2S_REQUIRE((h > 0) == (head != nullptr), "%s: head is given with h > 0 and only then", what);
    G2S_REQUIRE(S <= 32768, "%s: S too large", what);
    G2S_REQUIRE((long)h + 2l * b < (1l << 31), "%s: too many output rows", what);
    G2S_REQUIRE(rows < (1l << 40) / (3l * S * S) + 1, "%s: bank too large", what);
    BankGatherParams p;
    p.bank_img = bank_img, p.bank_mask = bank_mask, p.head = head;
    p.out_img = out_img, p.out_mask = out_mask, p.idx = idx, p.err = err;
    p.row_mask = (long)S * S, p.row_img = 3 * p.row_mask;
    p.rows = rows, p.b = b, p.h = h, p.idx64 = idx64 ? 1 : 0;
    p.vec_img = p.row_img % 4 == 0 && bg_aligned(bank_img, out_img, head);
    p.vec_mask = p.row_mask % 4 == 0 && bg_aligned(bank_mask, out_mask, nullptr);
    const long units = p.vec_img ? p.row_img / 4 : p.row_img;       // the longest row of the launch
    const long span = (long)BG_THREADS * BG_PER_THREAD;
    const long chunks = (units + span - 1) / span;
    dim3 grid((unsigned)(h + 2 * b), (unsigned)(chunks < BG_MAX_CHUNKS ? chunks : BG_MAX_CHUNKS));
    bank_gather_kernel<<<grid, BG_THREADS, 0, as_stream(stream)>>>(p);
    return check_launch(what);
}
