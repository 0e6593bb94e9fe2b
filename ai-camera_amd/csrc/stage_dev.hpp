// stage_dev.hpp -- the small device helpers of the analytics kernels, each once (device code only; included by kernels_zones.hip,
// kernels_bestshot.hip, kernels_colours.hip, kernels_scene.hip, kernels_left.hip and slot_walk.hpp).
// Integer arithmetic only.
#pragma once
#include "common.hpp"

namespace aic {
namespace {

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = imax(v, __shfl_xor(v, d));
    return v;
}

// a row's coordinate inside the stage's range; a row the stage looks at
__device__ __forceinline__ bool coord_ok(int v, int max) { return v >= -max && v <= max; }
__device__ __forceinline__ bool row_valid(int x1, int y1, int x2, int y2, int max) {
    return coord_ok(x1, max) && coord_ok(y1, max) && coord_ok(x2, max) && coord_ok(y2, max) && x2 >= x1 && y2 >= y1;
}

// exclusive prefix sum over the 512 threads of the block; total = the block's sum.  s_w: 8 ints of LDS, free again on return
__device__ __forceinline__ int block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int t = s_w[i];
        base += i < w ? t : 0;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

}  // namespace
}  // namespace aic
