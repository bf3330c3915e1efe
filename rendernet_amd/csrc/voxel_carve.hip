// Voxel carving: a grid from silhouettes and depth maps, the inverse of the ray caster under the rasteriser's integer camera
// (gfx950).  The rule -- which pixel a voxel's centre falls into, when a view is consistent with the voxel, the limits and the
// bounds -- is stated in include/rendernet_hip.h (rn_voxel_carve, rn_hit_depth); the NumPy twin is tests/voxel_carve_ref.py.
// Built with -ffp-contract=off: hit_depth_kernel is float64 and rounds every operation on its own, as the twin reads it; the
// carve is integer.
//
//   hit_depth_kernel    thread = pixel (the 16 x 16 tile grid of raycast_common.h): the caster's ray parameter t at the face it
//                       entered the hit voxel by, re-derived from (hit, face, m_inv), as a depth in 1/256 camera cell.
//   voxel_carve_kernel  thread = voxel, one launch: the loop over the K views runs inside, every thread counts its consistent
//                       views and stores one byte.  No atomics and nothing to clear: votes is a function of the input alone.
//                       The camera of (item, view) is the same for the whole workgroup: its address depends on blockIdx and
//                       the loop counter only, so the twelve words come through the scalar data cache into scalar registers,
//                       and so does the affine value of the workgroup's origin voxel (a . q_origin + b, three rows).  A lane
//                       adds its offset from that origin, a multiple of 256 a per axis -- exact in int64, the same integer as
//                       the full a . q + b -- and finishes with mesh_project.h's rounding shift and clamps.
//                       Lane -> voxel: a workgroup takes four 4 x 4 x 4 bricks side by side along xs, one per wave.  A brick's
//                       footprint on a view is a compact patch of pixels, where 64 voxels in a row leave a 64-voxel diagonal;
//                       the mapping cannot change the result, and DESIGN.md Appendix A has the timing of both.
#include "voxel_common.h"
#include "raycast_common.h"
#include "mesh_project.h"

namespace {

constexpr int kMaxViews = 255;            // votes is a byte
constexpr int kMaxSlack = 65535;
constexpr int kMaxViewSets = 65535;       // B K: (item, view) pairs of one call

// ---- entry depth of a caster hit ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void hit_depth_kernel(const int* __restrict__ hit_id, const signed char* __restrict__ face, const float* __restrict__ m_inv,
                      int* __restrict__ depth, int S, int N, int f, int row0, int col0, int ph, int pw, int low_x)
{
    const int b = blockIdx.z;
    const int pr = blockIdx.y * kTile + threadIdx.x / kTile, pc = blockIdx.x * kTile + threadIdx.x % kTile;
    if (pr >= ph || pc >= pw) return;
    const size_t o = ((size_t)b * ph + pr) * pw + pc;
    const int hit = hit_id[o], fc = face[o];
    int d = -1;
    if (hit >= 0 && hit < S * S * S && fc >= 0 && fc <= 5) {
        const int k = fc >> 1;
        const float* Mf = m_inv + (size_t)b * 12 + 4 * k;
        const double m0 = (double)Mf[0], m1 = (double)Mf[1], m2 = (double)Mf[2], m3 = (double)Mf[3];
        const double fd = (double)f;
        const double y = (double)(N - 1) - (((double)(row0 + pr) + 0.5) / fd - 0.5);
        const double z = ((double)(col0 + pc) + 0.5) / fd - 0.5;
        const double x0 = low_x ? -0.5 : (double)N - 0.5;
        const double ok = ((m0 * x0 + m1 * y) + m2 * z) + m3;
        const double dk = low_x ? m0 : -m0;
        const int vk = k == 0 ? hit % S : (k == 1 ? (hit / S) % S : hit / (S * S));
        const double plane = (fc & 1) ? (double)vk + 0.5 : (double)vk - 0.5;
        double t = dk == 0.0 ? 0.0 : (plane - ok) / dk;
        if (!(t == t)) t = 0.0;                                   // not a number (a matrix that is not finite): as d_k == 0
        const double u = floor(256.0 * (t > 0.0 ? t : 0.0));
        const double top = 256.0 * (double)N;
        d = (int)(u < 0.0 ? 0.0 : (u > top ? top : u));
    }
    depth[o] = d;
}

// ---- carve ----------------------------------------------------------------------------------------------------------------------

// the workgroup's origin voxel and this thread's offset from it, both (z, y, x): 16 x 4 x 4 (x, y, z) voxels, brick = wave, x fastest
template <int S>
__device__ __forceinline__ void carve_mapping(int block, int t, int org[3], int off[3])
{
    constexpr int kBx = S / 16, kBy = S / 4;
    org[2] = 16 * (block % kBx);
    org[1] = 4 * ((block / kBx) % kBy);
    org[0] = 4 * (block / (kBx * kBy));
    off[2] = (t & 3) + 4 * (t >> 6);
    off[1] = (t >> 2) & 3;
    off[0] = (t >> 4) & 3;
}

template <int S>
__global__ __launch_bounds__(kBlock)
void voxel_carve_kernel(const int* __restrict__ views, const i64* __restrict__ cam, unsigned char* __restrict__ votes, int K,
                        int row0, int col0, int ph, int pw, int use_depth, int slack, int outside_keep)
{
    const int b = blockIdx.y;
    int org[3], off[3];
    carve_mapping<S>((int)blockIdx.x, (int)threadIdx.x, org, off);
    const i64 q0 = 256 * org[0] + 128, q1 = 256 * org[1] + 128, q2 = 256 * org[2] + 128;     // uniform: the origin's centre
    const i64 d0 = 256 * off[0], d1 = 256 * off[1], d2 = 256 * off[2];                       // per lane, < 2^12
    const size_t view_px = (size_t)ph * pw;
    int count = 0;
    for (int k = 0; k < K; ++k) {
        const i64* __restrict__ c = cam + ((size_t)b * K + k) * 12;                         // uniform address
        i64 P[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const i64 base = c[4 * r] * q0 + c[4 * r + 1] * q1 + c[4 * r + 2] * q2 + c[4 * r + 3];
            P[r] = project_finish(base + c[4 * r] * d0 + c[4 * r + 1] * d1 + c[4 * r + 2] * d2, r);
        }
        const int pr = (int)(P[1] >> 8) - row0, pc = (int)(P[0] >> 8) - col0;               // floor: |X|, |Y| <= 2^20
        bool ok = outside_keep != 0;
        if ((unsigned)pr < (unsigned)ph && (unsigned)pc < (unsigned)pw) {                   // the bounds test of the one load
            const int v = views[((size_t)b * K + k) * view_px + (size_t)pr * pw + pc];
            ok = v >= 0 && (!use_depth || P[2] + slack >= (i64)v);
        }
        count += ok ? 1 : 0;
    }
    const int z = org[0] + off[0], y = org[1] + off[1], x = org[2] + off[2];
    votes[(size_t)b * S * S * S + ((size_t)z * S + y) * S + x] = (unsigned char)count;      // K <= 255
}

template <int S>
void launch_carve(const int* views, const i64* cam, unsigned char* votes, int B, int K, int row0, int col0, int ph, int pw,
                  int use_depth, int slack, int outside_keep, hipStream_t st)
{
    hipLaunchKernelGGL(voxel_carve_kernel<S>, dim3((unsigned)(S * S * S / kBlock), (unsigned)B), dim3(kBlock),
                       0, st, views, cam, votes, K, row0, col0, ph, pw, use_depth, slack, outside_keep);
}

}  // namespace

extern "C" int rn_hit_depth(const int* hit_id, const signed char* face, const float* m_inv, int* depth, int B, int S, int N,
                            int pixels_per_cell, int row0, int col0, int ph, int pw, int view_from_low_x, void* stream)
{
    const char* what = __func__;
    if (rn_check_grid_side_pow2(what, S) || rn_check_frame(what, B, N, pixels_per_cell, row0, col0, ph, pw)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {hit_id, face, m_inv, depth}) || rn_check_aligned(what, hit_id, 4, "hit_id") ||
        rn_check_aligned(what, m_inv, 4, "m_inv") || rn_check_aligned(what, depth, 4, "depth"))
        return RN_E_INVALID;
    hipLaunchKernelGGL(hit_depth_kernel, rn_tile_grid(B, ph, pw), dim3(kBlock), 0, (hipStream_t)stream, hit_id, face, m_inv, depth,
                       S, N, pixels_per_cell, row0, col0, ph, pw, view_from_low_x ? 1 : 0);
    return rn_check_launch(what);
}

extern "C" int rn_voxel_carve(const int* views, const long long* cam, unsigned char* votes, int B, int K, int S, int N,
                              int pixels_per_cell, int row0, int col0, int ph, int pw, int use_depth, int slack, int outside_keep,
                              void* stream)
{
    const char* what = __func__;
    if (rn_check_grid_side_pow2(what, S) || rn_check_frame(what, B, N, pixels_per_cell, row0, col0, ph, pw)) return RN_E_INVALID;
    if (K < 1 || K > kMaxViews) return rn_set_error(RN_E_INVALID, "%s: K=%d views (1..%d: votes is a byte)", what, K, kMaxViews);
    if ((long long)B * K > kMaxViewSets)
        return rn_set_error(RN_E_INVALID, "%s: B K = %lld (item, view) pairs (at most %d per call)", what, (long long)B * K, kMaxViewSets);
    if (slack < 0 || slack > kMaxSlack) return rn_set_error(RN_E_INVALID, "%s: slack=%d (0..%d)", what, slack, kMaxSlack);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {views, cam, votes}) || rn_check_aligned(what, views, 4, "views") || rn_check_aligned(what, cam, 8, "cam"))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int ud = use_depth ? 1 : 0, keep = outside_keep ? 1 : 0;
    const i64* c = (const i64*)cam;
    if (S == 32) launch_carve<32>(views, c, votes, B, K, row0, col0, ph, pw, ud, slack, keep, st);
    else if (S == 64) launch_carve<64>(views, c, votes, B, K, row0, col0, ph, pw, ud, slack, keep, st);
    else launch_carve<128>(views, c, votes, B, K, row0, col0, ph, pw, ud, slack, keep, st);
    return rn_check_launch(what);
}
