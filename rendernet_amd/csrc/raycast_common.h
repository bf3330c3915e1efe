// What the second stages of the voxel ray caster share (raycast.hip, raycast_albedo.hip): the pixel tile, the masked
// window sum of the three encode kernels, and the argument checks of the entry points, each stated once.
// raycast.hip is built with -ffp-contract=off and raycast_albedo.hip is not; everything here is integer, so both read the
// same code.
#pragma once
#include "rn_checks.h"

constexpr int kTile = 16;                 // pixel tile side of one 256-thread block
constexpr int kMaxSmooth = 8;             // largest radius of the window mean, in pixels
static_assert(kMaxSmooth == RN_ALBEDO_MAX_SMOOTH, "one maximum smoothing radius for every encode stage");

static inline dim3 rn_tile_grid(int B, int ph, int pw)
{
    return dim3((unsigned)((pw + kTile - 1) / kTile), (unsigned)((ph + kTile - 1) / kTile), (unsigned)B);
}

// The LDS of one block of an encode kernel, declared there as `__shared__ WindowCells<T> cell; __shared__ WindowRowSums<T>
// rowsum;`: its 16x16 tile with a halo of r <= kMaxSmooth pixels, one packed cell per pixel, and the sums of the cells along
// the rows.
constexpr int kWindowSide = kTile + 2 * kMaxSmooth;
template <typename Cell> using WindowCells = Cell[kWindowSide][kWindowSide + 1];
template <typename Cell> using WindowRowSums = Cell[kWindowSide][kTile];

// The masked sum over the (2r+1)^2 window, clipped to the [ph,pw] picture of item blockIdx.z, around this thread's pixel
// (row blockIdx.y * kTile + threadIdx.x / kTile, column blockIdx.x * kTile + threadIdx.x % kTile).  load(gr, gc) packs the
// pixel (gr, gc) of the picture into a cell: not 0 for a hit, with its values and a 1 for the count in separate bit fields
// wide enough for 289 terms, and 0 for a miss; pixels outside the picture are 0.  The tile and its halo are staged once, the
// window sum is taken along the rows, then along the columns.  Every thread of the block calls this and reaches both
// barriers; false for a thread whose pixel lies outside the picture, else `sum` is the window's and `centre` the pixel's own
// cell (not 0 means a hit, and then the count in `sum` is at least 1).
// The caller chooses how a halo pixel outside the picture becomes 0.  HaloLoad::predicated branches around load, which is
// then called for pixels of the picture only: for a load of several dependent reads (albedo).  HaloLoad::clamped has no
// branch: load is ALSO called for the nearest pixel inside, and its result dropped: for a load of one byte (AO, shadow),
// where the branch costs more than the read; such a load must be free of side effects.
enum class HaloLoad { predicated, clamped };

template <HaloLoad kHalo, typename Cell, typename Load>
__device__ __forceinline__ bool window_sum(WindowCells<Cell>& cell, WindowRowSums<Cell>& rowsum, int ph, int pw, int r, Load load,
                                           Cell& sum, Cell& centre)
{
    const int r0 = blockIdx.y * kTile - r, c0 = blockIdx.x * kTile - r, w = kTile + 2 * r;
    for (int i = threadIdx.x; i < w * w; i += 256) {
        const int y = i / w, x = i - y * w, gr = r0 + y, gc = c0 + x;
        const bool inside = gr >= 0 && gr < ph && gc >= 0 && gc < pw;
        if (kHalo == HaloLoad::clamped) {
            const Cell v = load(min(max(gr, 0), ph - 1), min(max(gc, 0), pw - 1));
            cell[y][x] = inside ? v : Cell(0);
        } else {
            cell[y][x] = inside ? load(gr, gc) : Cell(0);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < w * kTile; i += 256) {
        const int y = i / kTile, x = i % kTile;
        Cell s = 0;
        for (int dx = 0; dx <= 2 * r; ++dx) s += cell[y][x + dx];
        rowsum[y][x] = s;
    }
    __syncthreads();
    const int ty = threadIdx.x / kTile, tx = threadIdx.x % kTile;
    const int pr = blockIdx.y * kTile + ty, pc = blockIdx.x * kTile + tx;
    if (pr >= ph || pc >= pw) return false;
    sum = 0;
    for (int dy = 0; dy <= 2 * r; ++dy) sum += rowsum[ty + dy][tx];
    centre = cell[ty + r][tx + r];
    return true;
}

// The argument checks only the ray caster's entry points make, in the style of rn_checks.h, which has the general ones
// (batch, pointers, alignment).  The tools' rn_check_grid_side_pow2 does not take 96.
static inline int rn_check_grid_side_x32(const char* what, int S)
{
    return (S < 32 || S > 128 || S % 32 != 0) ? rn_set_error(RN_E_INVALID, "%s: S=%d (a multiple of 32 up to 128)", what, S)
                                              : RN_OK;
}

static inline int rn_check_window(const char* what, int ph, int pw)
{
    return (ph < 1 || pw < 1 || ph > 4096 || pw > 4096)
               ? rn_set_error(RN_E_INVALID, "%s: window %dx%d (1..4096 each way)", what, ph, pw) : RN_OK;
}

static inline int rn_check_smooth(const char* what, int smooth)
{
    return (smooth < 0 || smooth > kMaxSmooth) ? rn_set_error(RN_E_INVALID, "%s: smooth=%d (0..%d)", what, smooth, kMaxSmooth)
                                               : RN_OK;
}

static inline int rn_check_quantised_light(const char* what, int lx, int ly, int lz)
{
    return (lx < -32767 || lx > 32767 || ly < -32767 || ly > 32767 || lz < -32767 || lz > 32767)
               ? rn_set_error(RN_E_INVALID, "%s: light (%d, %d, %d), each component within +-32767", what, lx, ly, lz) : RN_OK;
}

// the three int32 inputs of a second stage that walks the grid from given hits: the mask is copied as uint4
static inline int rn_check_hit_alignment(const char* what, const unsigned* bits, const int* box, const int* hit_id)
{
    return (((uintptr_t)bits & 15) != 0 || ((uintptr_t)box & 3) != 0 || ((uintptr_t)hit_id & 3) != 0)
               ? rn_set_error(RN_E_INVALID, "%s: bits must be 16-byte aligned, box and hit_id 4-byte aligned", what) : RN_OK;
}
