// wave_sum.h — the sum of one value per lane over a 64-lane wavefront, left in every lane.
// A butterfly of __shfl_xor: the order of the additions is fixed, so the result repeats bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace g2s {

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace g2s
