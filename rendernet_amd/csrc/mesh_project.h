// The projection of the integer camera, stated once for the two files that project with it: mesh_raster.hip (the vertices of a
// mesh) and voxel_carve.hip (the centres of a grid's voxels).  include/rendernet_hip.h (rn_mesh_rasterize) states the rule and
// derives the bounds: |a . q + b| < 2^61 for lattice points q in [0, 256 S]^3, so everything fits signed 64-bit.  Integer only:
// the files that include it are built with -ffp-contract=off, which this code does not notice.
#pragma once

typedef long long i64;
typedef unsigned long long u64;

constexpr int kFix = 20;                                         // cam is 2^20 fixed point
constexpr i64 kClampXY = 1ll << 20, kClampZ = 1ll << 17;

__device__ __forceinline__ i64 clampi(i64 x, i64 lo, i64 hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The last two steps of the projection, on the affine value s = a . q + b of camera row r (0, 1, 2 = 256 X, 256 Y, 256 D): the
// rounding shift, then the clamp -- X and Y to +-2^20, the depth to +-2^17.  A caller that forms s some other way than
// project_row (voxel_carve.hip adds per-lane multiples of a to a wave's origin: the same integer, int64 arithmetic is exact)
// comes through here, so there is one statement of the rounding and the clamps.
__device__ __forceinline__ i64 project_finish(i64 s, int r)
{
    const i64 v = (s + (1ll << (kFix - 1))) >> kFix;
    return r == 2 ? clampi(v, -kClampZ, kClampZ) : clampi(v, -kClampXY, kClampXY);
}

// coordinate r of lattice point (q0, q1, q2) (array-axis order) under cam [3][4]
__device__ __forceinline__ i64 project_row(const i64* __restrict__ cam, int r, i64 q0, i64 q1, i64 q2)
{
    return project_finish(cam[4 * r] * q0 + cam[4 * r + 1] * q1 + cam[4 * r + 2] * q2 + cam[4 * r + 3], r);
}
