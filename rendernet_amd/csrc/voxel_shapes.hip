// Procedural voxel shapes: occupancy grids rasterised from a seeded constructive-solid-geometry description (gfx950), the
// geometry source of the synthetic training feeds.  The grid is a deterministic INTEGER function of the description; the
// rule, its clamps and the bounds that keep every intermediate inside 32 / 64 bits are stated in include/rendernet_hip.h
// (rn_voxel_shapes), the NumPy twin is tests/voxel_shapes_ref.py.  No float appears in this file.
//
//   voxel_shapes_kernel  a thread rasterises kRun = 16 consecutive xs of one row and writes them with one 128-bit store; a
//                    256-thread block covers 4096 consecutive voxels of one item (a z slice at S = 64, four at S = 32).
//                    The item's primitives (512 bytes, uniform across the block) are read once, 128 bits per thread, clamped,
//                    and staged in LDS with the ellipsoid weights 2^14 / a; every lane then reads the same row (an LDS
//                    broadcast), and the branch on the primitive's type is uniform.  q is linear in xs: along its run a thread
//                    adds 2 R_i0 (and 2 w_i R_i0) in 32 bits; only the squares are 64-bit products.
#include "rn_checks.h"

namespace {

constexpr int kRun = 16;                          // consecutive xs per thread
constexpr int kBlockVoxels = 256 * kRun;
constexpr long long kUnit = 64ll << 14;           // the ellipsoid's radius in units of w q
// staged primitive: words 0..15 as the header lists them, clamped (word 0 = type | op << 8, or -1 for a no-op), 16..18 = w
constexpr int kWords = 20;

__device__ __forceinline__ long long sq(int v) { return (long long)v * v; }

__global__ __launch_bounds__(256)
void voxel_shapes_kernel(const int4* __restrict__ prims, uint4* __restrict__ vox, int K, int S, int log2S)
{
    __shared__ int sp[RN_SHAPES_MAX_PRIMS][kWords];
    const int b = blockIdx.y, t = threadIdx.x;
    if (t < K * 4) {                                              // K <= 8: the first 32 lanes, one 128-bit read each
        const int4 v = prims[(size_t)b * K * 4 + t];
        const int k = t >> 2, j0 = (t & 3) * 4;
        const int word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = j0 + i;
            int x = word[i];
            if (j == 0) {
                const int type = x & 255, op = x >> 8;
                x = (type <= 4 && (op == 0 || op == 1)) ? (type | op << 8) : -1;
            } else if (j >= 4 && j <= 6) {
                x = min(max(x, 1), 128);
                sp[k][16 + j - 4] = 16384 / x;
            } else {
                x = min(max(x, -64), 64);
            }
            sp[k][j] = x;
        }
    }
    __syncthreads();

    const int i0 = (blockIdx.x * 256 + t) * kRun;                 // flat index of the run's first voxel, < S^3 (S^3 % 4096 == 0)
    const int xs0 = i0 & (S - 1), ys = (i0 >> log2S) & (S - 1), zs = i0 >> (2 * log2S);
    const int Px = 2 * xs0 - (S - 1), Py = 2 * ys - (S - 1), Pz = 2 * zs - (S - 1);
    unsigned occ = 0;                                             // bit j = voxel xs0 + j
    for (int k = 0; k < K; ++k) {
        const int* p = sp[k];
        const int head = p[0];
        if (head < 0) continue;                                   // uniform across the block, like the switch below
        const int dx = Px - p[1], dy = Py - p[2], dz = Pz - p[3];
        int q0 = p[7] * dx + p[8] * dy + p[9] * dz;
        int q1 = p[10] * dx + p[11] * dy + p[12] * dz;
        int q2 = p[13] * dx + p[14] * dy + p[15] * dz;
        const int s0 = 2 * p[7], s1 = 2 * p[10], s2 = 2 * p[13];  // q of the next voxel along xs
        const int A0 = 64 * p[4], A1 = 64 * p[5], A2 = 64 * p[6];
        unsigned m = 0;
        switch (head & 255) {
        case 0: {                                                 // ellipsoid
            int u0 = p[16] * q0, u1 = p[17] * q1, u2 = p[18] * q2;
            const int t0 = p[16] * s0, t1 = p[17] * s1, t2 = p[18] * s2;
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                m |= (unsigned)(sq(u0) + sq(u1) + sq(u2) <= kUnit * kUnit) << j;
                u0 += t0; u1 += t1; u2 += t2;
            }
        } break;
        case 1:                                                   // box
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                m |= (unsigned)(abs(q0) <= A0 && abs(q1) <= A1 && abs(q2) <= A2) << j;
                q0 += s0; q1 += s1; q2 += s2;
            }
            break;
        case 2: {                                                 // cylinder
            int u0 = p[16] * q0, u1 = p[17] * q1;
            const int t0 = p[16] * s0, t1 = p[17] * s1;
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                m |= (unsigned)(sq(u0) + sq(u1) <= kUnit * kUnit && abs(q2) <= A2) << j;
                u0 += t0; u1 += t1; q2 += s2;
            }
        } break;
        case 3: {                                                 // cone
            const int f = 4 * A2 * A2;
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                m |= (unsigned)(abs(q2) <= A2 && (long long)f * (q0 * q0 + q1 * q1) <= sq(A0 * (A2 - q2))) << j;
                q0 += s0; q1 += s1; q2 += s2;
            }
        } break;
        default: {                                                // 4: torus
            const int f = 4 * A0 * A0, g = A0 * A0 - A1 * A1;
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                const int s = q0 * q0 + q1 * q1, l = s + q2 * q2 + g;
                m |= (unsigned)(l <= 0 || sq(l) <= (long long)f * s) << j;
                q0 += s0; q1 += s1; q2 += s2;
            }
        } break;
        }
        occ = (head >> 8) ? occ & ~m : occ | m;
    }
    // four bits -> four bytes of 0 / 1: bit k lands on bit 8k through the term 2^(7k); no two terms meet, so nothing carries
    uint4 o;
    o.x = ((occ & 15u) * 0x00204081u) & 0x01010101u;
    o.y = (((occ >> 4) & 15u) * 0x00204081u) & 0x01010101u;
    o.z = (((occ >> 8) & 15u) * 0x00204081u) & 0x01010101u;
    o.w = (((occ >> 12) & 15u) * 0x00204081u) & 0x01010101u;
    vox[(size_t)b * ((size_t)S * S * S / kRun) + blockIdx.x * 256 + t] = o;
}

}  // namespace

extern "C" int rn_voxel_shapes(const int* prims, unsigned char* vox, int B, int K, int S, void* stream)
{
    if (rn_check_batch_sign(__func__, B)) return RN_E_INVALID;
    if (K < 0 || K > RN_SHAPES_MAX_PRIMS)
        return rn_set_error(RN_E_INVALID, "rn_voxel_shapes: K=%d (0..%d primitives)", K, RN_SHAPES_MAX_PRIMS);
    if (S != 32 && S != 64)
        return rn_set_error(RN_E_INVALID, "rn_voxel_shapes: S=%d (32 or 64: the rule's 32-bit bounds end at 64)", S);
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {vox}) || (K > 0 && rn_check_pointers(__func__, {prims})) ||
        rn_check_aligned(__func__, prims, 16, "prims") || rn_check_aligned(__func__, vox, 16, "vox"))
        return RN_E_INVALID;
    static_assert(32 * 32 * 32 % kBlockVoxels == 0, "whole blocks at both sizes");
    const dim3 grid((unsigned)(S * S * S / kBlockVoxels), (unsigned)B);
    hipLaunchKernelGGL(voxel_shapes_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const int4*)prims, (uint4*)vox, K, S,
                       S == 64 ? 6 : 5);
    return rn_check_launch("rn_voxel_shapes");
}
