// What the device code of the voxel and mesh tools shares (voxel_edt.hip, voxel_label.hip, mesh_extract.hip, mesh_voxel.hip,
// mesh_raster.hip, image_metrics.hip): the workgroup shape, the fixed-order block sum, stream compaction without atomics, the
// row word of a packed grid and the floor division, each stated once.  Some of those files are built with -ffp-contract=off
// and some are not; the one floating-point expression here is a sum, which has nothing to contract.
#pragma once
#include "rn_common.h"

constexpr int kBlock = 256;               // threads of a workgroup
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
static_assert(kWaves == 4, "block_sum, block_count and block_rank spell out the sum of four waves");

__device__ __forceinline__ long long floor_div(long long n, long long d)      // d > 0
{
    const long long q = n / d;
    return (n % d < 0) ? q - 1 : q;
}

// Word w of row (z, y) of a packed S^3 occupancy grid (bit x & 31 of word x >> 5 is voxel x of the row); 0 outside the grid.
// This is the PLAIN word.  A caller that wants the empty space complements it itself, because where it does so is its rule:
// voxel_edt.hip after this bounds check (the outside is empty, hence a seed), voxel_label.hip inside it (the outside selects
// nothing).
template <int S>
__device__ __forceinline__ bool word_outside(int z, int y, int w)
{
    return (unsigned)z >= (unsigned)S || (unsigned)y >= (unsigned)S || (unsigned)w >= (unsigned)(S / 32);
}

template <int S>
__device__ __forceinline__ unsigned occ_word(const unsigned* __restrict__ g, int z, int y, int w)
{
    if (word_outside<S>(z, y, w)) return 0u;
    return g[(z * S + y) * (S / 32) + w];
}

// The sum of v over the workgroup, in every thread; `red` is kWaves words of LDS.  The order of the additions is fixed and is
// part of the contract -- down the wave by 32, 16, .. 1, then ((wave 0 + wave 1) + wave 2) + wave 3 -- because image_metrics.hip
// sums float64 terms with it and its tests compare the result with a twin that adds in this order, bit for bit.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                                             // red may still be read from the previous sum
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- stream compaction: every item gets its index in the output without an atomic, so the order is the order of the threads ----
// Three launches.  Count: each workgroup writes how many items it has (block_count).  Scan: one workgroup per grid turns the
// workgroup totals into their exclusive prefixes and returns the grid's total (scan_totals).  Emit: the same votes again, the
// index of a lane's first item is its workgroup's prefix + block_rank.  A lane's items are a predicate (__ballot, __popcll,
// lanes_before) or a count of 0..3 (Vote2).  Every thread of the workgroup calls these: they hold barriers.

__device__ __forceinline__ int lanes_before(unsigned long long ballot)      // set bits below this lane
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

struct Vote2 { unsigned long long b0, b1; };                     // the ballots of the two bits of a per-lane count of 0..3
__device__ __forceinline__ Vote2 vote2(int n) { return {__ballot(n & 1), __ballot(n & 2)}; }
__device__ __forceinline__ int wave_total(Vote2 v) { return __popcll(v.b0) + 2 * __popcll(v.b1); }
__device__ __forceinline__ int lanes_before(Vote2 v) { return lanes_before(v.b0) + 2 * lanes_before(v.b1); }

// the items of the workgroup, from each wave's; T is int, or int2 for two counts behind one barrier; `sw` is kWaves T of LDS
template <typename T>
__device__ __forceinline__ T block_count(T in_wave, T* sw)
{
    if ((threadIdx.x & (kWave - 1)) == 0) sw[threadIdx.x / kWave] = in_wave;
    __syncthreads();
    return ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// the index of this lane's first item among the workgroup's: the waves before this one, the lanes before this one.  The index
// in the output is the workgroup's prefix, which scan_totals left, plus this
__device__ __forceinline__ int block_rank(int in_wave, int in_lanes_before, int* sw)
{
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) sw[wave] = in_wave;
    __syncthreads();
    int rank = in_lanes_before;
#pragma unroll
    for (int j = 0; j < kWaves - 1; ++j)
        if (j < wave) rank += sw[j];
    return rank;
}

__device__ __forceinline__ int shfl_up_each(int v, int d) { return __shfl_up(v, d); }
__device__ __forceinline__ int2 shfl_up_each(int2 v, int d) { return make_int2(__shfl_up(v.x, d), __shfl_up(v.y, d)); }

// w[0 .. nb) becomes its exclusive prefix sums in place; returns the total.  T is int or int2 (two counts scanned together);
// `swave` is kWaves T of LDS.  256 totals a round: a shuffle scan in the wave, LDS across the four waves, a running carry.
template <typename T>
__device__ __forceinline__ T scan_totals(T* w, int nb, T* swave)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    T carry = T();
    for (int base = 0; base < nb; base += kBlock) {              // nb is uniform: every thread reaches both barriers
        const int k = base + threadIdx.x;
        const T x = k < nb ? w[k] : T();
        T inc = x;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const T t = shfl_up_each(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == kWave - 1) swave[wave] = inc;
        __syncthreads();
        T pre = carry;
#pragma unroll
        for (int j = 0; j < kWaves; ++j) {
            if (j < wave) pre += swave[j];
            carry += swave[j];
        }
        if (k < nb) w[k] = pre + inc - x;
        __syncthreads();                                         // swave is rewritten by the next round
    }
    return carry;
}
