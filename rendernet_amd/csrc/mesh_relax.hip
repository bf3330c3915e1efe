// Surface-net relaxation: the second half of SurfaceNets on the vertices rn_mesh_extract_emit wrote (gfx950).  Every vertex
// moves towards the mean of its linked neighbours and stays inside its own cell, so faces, order and the solid round trip are
// what they were.  The rule -- cell, bounds, links, the pass -- is stated once in include/rendernet_hip.h (rn_mesh_relax); the
// NumPy twin is tests/mesh_relax_ref.py, which takes its links from the quad rings where this file takes them from the corner
// bits.  Integer arithmetic throughout: the inside test is a comparison, so the file needs no floating-point flag.
//
// One thread per VERTEX (a grid has some thousands of them in (S + 1)^3 cells), 256-thread workgroups, no atomics and nothing
// that waits for another workgroup: the passes are separate launches over two buffers.
//
//   relax_links_kernel   the vertex's grid by bisection of vert_offsets, its cell from its coordinates, the cell's 8-corner mask
//                        from the volume (mesh_cells.h: the extractor's inside test and virtual samples), the six link bits from
//                        the mask's faces, and the linked cells' vertex ids from the cell->vertex volume: one row of six GLOBAL
//                        vertex indices (-1: no link) in the workspace.  With an odd number of passes it also copies the vertex
//                        to the second buffer, where the first pass then reads it, so that the last pass always writes q.
//   relax_pass_kernel    one Jacobi pass: the row, the linked vertices of the source buffer, the rule, the other buffer.
//
// Bounds.  The grid is searched inside 0 .. B-1 and the cell is clamped to [-1, S-1]^3 whatever q and vert_offsets hold; a link
// towards c_a = -2 or S cannot arise (those corners are virtual, hence all outside) and is tested all the same; a neighbour's
// global index is tested against [0, n_verts) before it enters the table.  So no content of q, vert_offsets, cellvert or the
// volume makes a kernel touch memory outside its arrays, and the pass kernel reads only indices the links kernel vouched for.
#include "voxel_common.h"
#include "mesh_cells.h"
#include "rn_checks.h"

namespace {

constexpr int kLinks = 6;                                        // (-e0, +e0, -e1, +e1, -e2, +e2)
constexpr int kMaxPasses = 64;
constexpr int kMaxWeight = 256;

// the corners of a cell (bit 4 b0 + 2 b1 + b2) with b_a = 0 and with b_a = 1
__device__ __forceinline__ unsigned face_bits(int a, int side)
{
    const unsigned low = a == 0 ? 0x0fu : a == 1 ? 0x33u : 0x55u;
    return side ? low ^ 0xffu : low;
}

__device__ __forceinline__ int cell_index(int q, int S) { return min(max(((q + 128) >> 8) - 1, -1), S - 1); }

template <typename T>
__global__ __launch_bounds__(kBlock)
void relax_links_kernel(const T* __restrict__ vol, float threshold, int B, int S, const int* __restrict__ cellvert,
                        const long long* __restrict__ vert_offsets, long long n_verts, const int* __restrict__ q,
                        int* __restrict__ links, int* __restrict__ copy)
{
    const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_verts) return;
    int lo = 0, hi = B - 1;                                      // the last b with vert_offsets[b] <= g, inside 0 .. B-1
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (vert_offsets[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int b = lo, N = S + 1;
    const int p[3] = {q[3 * g], q[3 * g + 1], q[3 * g + 2]};
    if (copy) {
#pragma unroll
        for (int a = 0; a < 3; ++a) copy[3 * g + a] = p[a];
    }
    const int c[3] = {cell_index(p[0], S), cell_index(p[1], S), cell_index(p[2], S)};
    const unsigned mask = corner_mask<T, false>(vol + (size_t)b * S * S * S, S, threshold, Cell{c[0], c[1], c[2]}, nullptr);
    const int* cv = cellvert + (size_t)b * N * N * N;
    const int cell = ((c[0] + 1) * N + (c[1] + 1)) * N + (c[2] + 1);
    const int stride[3] = {N * N, N, 1};
    const long long base = vert_offsets[b];
    int row[kLinks];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const unsigned face = face_bits(a, side), in = mask & face;
            const int ca = c[a] + (side ? 1 : -1);
            int id = -1;
            if (in != 0u && in != face && ca >= -1 && ca <= S - 1) {
                const int word = cv[cell + (side ? stride[a] : -stride[a])];
                const long long at = base + (word & kIdMask);
                if (word >= 0 && at >= 0 && at < n_verts) id = (int)at;                            // n_verts < 2^31
            }
            row[2 * a + side] = id;
        }
    }
    int2* out = (int2*)(links + kLinks * g);                     // 24 bytes a row
    out[0] = make_int2(row[0], row[1]);
    out[1] = make_int2(row[2], row[3]);
    out[2] = make_int2(row[4], row[5]);
}

__global__ __launch_bounds__(kBlock)
void relax_pass_kernel(const int* __restrict__ links, const int* __restrict__ src, int* __restrict__ dst, long long n_verts, int S,
                       int weight)
{
    const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_verts) return;
    const int2* in = (const int2*)(links + kLinks * g);
    const int2 r0 = in[0], r1 = in[1], r2 = in[2];
    const int row[kLinks] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y};
    int sum[3] = {0, 0, 0}, n = 0;
#pragma unroll
    for (int k = 0; k < kLinks; ++k) {
        if (row[k] < 0) continue;
        const int* s = src + 3 * (long long)row[k];
        sum[0] += s[0];
        sum[1] += s[1];
        sum[2] += s[2];
        ++n;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int p = src[3 * g + a];
        int t = p;                                               // no link: the vertex stays where it is
        if (n > 0) {
            const int c = cell_index(p, S);
            // 256 n p + w (sum - n p) + 128 n, every term non-negative in this form: below 2^27, so / is floor
            t = ((256 - weight) * n * p + weight * sum[a] + 128 * n) / (256 * n);
            t = min(max(t, max(0, 256 * c + 129)), min(256 * S, 256 * c + 383));
        }
        dst[3 * g + a] = t;
    }
}

size_t links_bytes(long long n_verts) { return (size_t)n_verts * kLinks * sizeof(int); }

// 0 when n_verts is one the entries take
int check_verts(const char* who, long long n_verts)
{
    return (n_verts < 0 || n_verts > (1ll << 31) - 1) ? rn_set_error(RN_E_INVALID, "%s: n_verts=%lld (0..2^31 - 1)", who, n_verts) : RN_OK;
}

}  // namespace

extern "C" size_t rn_mesh_relax_workspace_bytes(long long n_verts)
{
    if (check_verts(__func__, n_verts)) return 0;
    return (links_bytes(n_verts) + (size_t)n_verts * 3 * sizeof(int) + 15) / 16 * 16;
}

extern "C" int rn_mesh_relax(const void* vol, int vol_is_u8, float threshold, int B, int S, const int* cellvert,
                             const long long* vert_offsets, long long n_verts, int passes, int weight, void* workspace,
                             size_t workspace_bytes, int* q, void* stream)
{
    const char* who = __func__;
    if (rn_check_grid_side_pow2(who, S) || rn_check_batch(who, B) || check_verts(who, n_verts)) return RN_E_INVALID;
    if (vol_is_u8 != 0 && vol_is_u8 != 1) return rn_set_error(RN_E_INVALID, "%s: vol_is_u8=%d", who, vol_is_u8);
    if (!(threshold == threshold)) return rn_set_error(RN_E_INVALID, "%s: threshold is NaN", who);
    if (passes < 0 || passes > kMaxPasses) return rn_set_error(RN_E_INVALID, "%s: passes=%d (0..%d)", who, passes, kMaxPasses);
    if (weight < 1 || weight > kMaxWeight) return rn_set_error(RN_E_INVALID, "%s: weight=%d (1..%d)", who, weight, kMaxWeight);
    if (B == 0 && n_verts != 0) return rn_set_error(RN_E_INVALID, "%s: %lld vertices of no grid", who, n_verts);
    if (B == 0 || n_verts == 0) return RN_OK;
    if (rn_check_pointers(who, {vol, cellvert, vert_offsets, q}) || rn_check_aligned(who, vol, vol_is_u8 ? 1 : 4, "vol") ||
        rn_check_aligned(who, cellvert, 4, "cellvert") || rn_check_aligned(who, vert_offsets, 8, "vert_offsets") ||
        rn_check_aligned(who, q, 4, "q") || rn_check_ws(who, workspace, workspace_bytes, rn_mesh_relax_workspace_bytes(n_verts)))
        return RN_E_INVALID;
    if (passes == 0) return RN_OK;
    hipStream_t st = (hipStream_t)stream;
    int* links = (int*)workspace;
    int* other = (int*)((char*)workspace + links_bytes(n_verts));
    const dim3 grid((unsigned)((n_verts + kBlock - 1) / kBlock)), block(kBlock);
    int* copy = (passes & 1) ? other : nullptr;                  // odd: the passes run other -> q -> .. -> q; even: q -> other -> .. -> q
    if (vol_is_u8)
        hipLaunchKernelGGL(relax_links_kernel<unsigned char>, grid, block, 0, st, (const unsigned char*)vol, threshold, B, S, cellvert,
                           vert_offsets, n_verts, q, links, copy);
    else
        hipLaunchKernelGGL(relax_links_kernel<float>, grid, block, 0, st, (const float*)vol, threshold, B, S, cellvert, vert_offsets,
                           n_verts, q, links, copy);
    int* src = copy ? other : q;
    int* dst = copy ? q : other;
    for (int k = 0; k < passes; ++k) {
        hipLaunchKernelGGL(relax_pass_kernel, grid, block, 0, st, links, src, dst, n_verts, S, weight);
        int* t = src;
        src = dst;
        dst = t;
    }
    return rn_check_launch(who);
}
