// The cells of the surface net, as mesh_extract.hip and mesh_relax.hip both read them (include/rendernet_hip.h states the rule):
// the cell of a flat index, the level of a sample, the 8-corner inside mask and the layout of a word of the cell->vertex volume.
// level() is one float32 subtract, multiply and rint, each rounded on its own: a file that instantiates corner_mask with
// kLevels = true is built with -ffp-contract=off (mesh_extract.hip); the mask alone is a comparison and needs no flag.
#pragma once
#include "rn_common.h"

namespace {

constexpr float kDmax = 4194304.f;                               // 2^22
constexpr int kIdBits = 24;                                      // 129^3 < 2^22 vertex ids
constexpr int kIdMask = (1 << kIdBits) - 1;

struct Cell { int c0, c1, c2; };                                 // each in [-1, S - 1]

__device__ __forceinline__ Cell cell_of(int i, int N)
{
    const int a = i / (N * N), r = i - a * N * N;
    return {a - 1, r / N - 1, r % N - 1};
}

// |D| of a sample value: clamp(rint((v - threshold) * 65536), -2^22, 2^22), float32, two roundings
__device__ __forceinline__ int level(float v, float threshold)
{
    const float d = rintf((v - threshold) * 65536.f);
    return (int)fabsf(fminf(fmaxf(d, -kDmax), kDmax));
}

// bit (4 b0 + 2 b1 + b2) = corner (c0 + b0, c1 + b1, c2 + b2) is inside; kLevels also fills |D| of the eight corners
template <typename T, bool kLevels>
__device__ __forceinline__ unsigned corner_mask(const T* __restrict__ grid, int S, float threshold, Cell c, int* __restrict__ lev)
{
    unsigned mask = 0;
    const int outside = kLevels ? level(0.f, threshold) : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s0 = c.c0 + (k >> 2), s1 = c.c1 + ((k >> 1) & 1), s2 = c.c2 + (k & 1);
        const bool real = (unsigned)s0 < (unsigned)S && (unsigned)s1 < (unsigned)S && (unsigned)s2 < (unsigned)S;
        if (kLevels) lev[k] = outside;
        if (real) {
            const float v = (float)grid[((size_t)s0 * S + s1) * S + s2];
            if (v > threshold) mask |= 1u << k;
            if (kLevels) lev[k] = level(v, threshold);
        }
    }
    return mask;
}

}  // namespace
