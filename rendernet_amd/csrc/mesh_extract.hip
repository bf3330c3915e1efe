// Surface-net mesh extraction: the quad mesh of a voxel grid on the voxeliser's 1/256-voxel lattice (gfx950), the mesh OUTPUT of
// the project.  The rule -- inside test, lattice, crossing, vertex, quads and their order -- is stated once in
// include/rendernet_hip.h (rn_mesh_extract_count / rn_mesh_extract_emit); the NumPy twin is tests/mesh_extract_ref.py.  Integer
// arithmetic apart from one float32 subtract, multiply and rint per sample; built with -ffp-contract=off so that the two stay
// two roundings as the twin's are.
//
// One thread per cell, 256-thread workgroups of four wave64s, grid (workgroups per grid, B).  No atomic decides an index: the
// vertices and the quads are numbered by the stream compaction of voxel_common.h (block_count, scan_totals, block_rank):
//
//   extract_count_kernel   the 8-corner inside mask of the cell; the workgroup's active cells and owned quads (0..3 per cell: a
//                          Vote2) go to the workspace as (vertices, quads)
//   extract_scan_kernel    one workgroup per grid leaves the exclusive prefixes of the workgroup totals in place; the total is
//                          the grid's (V, F), which the host reads back to size the outputs
//   extract_verts_kernel   same mask again; vertex id = the rank of the cell among the active ones.
//                          Writes the lattice vertex and, into the cell->vertex volume, id | flags << 24 (-1 for an inactive
//                          cell): flag bit a = the cell owns a quad about axis a, bit 3 + a = that edge's lower end is inside
//   extract_quads_kernel   reads only the cell->vertex volume: its own word for the flags, the three neighbours per owned quad
//                          for their ids; quad index = the rank of the cell's first quad
//
// A cell owns the edge from its corner (0,1,1) / (1,0,1) / (1,1,0) to its corner (1,1,1).  When c_u + 1 = S both ends are virtual
// samples, which are outside, so the edge never differs: the rule's "c_u + 1 <= S - 1" needs no test of its own here.
#include "voxel_common.h"
#include "mesh_cells.h"
#include "rn_checks.h"

namespace {

// bits 0..2: the cell owns a quad about axis 0, 1, 2; bits 3..5: the lower end of that edge is the inside one
__device__ __forceinline__ unsigned quad_flags(unsigned mask)
{
    const unsigned top = (mask >> 7) & 1u;
    const unsigned low = ((mask >> 3) & 1u) | (((mask >> 5) & 1u) << 1) | (((mask >> 6) & 1u) << 2);   // corners 011, 101, 110
    return (low ^ (top * 7u)) | (low << 3);
}

template <typename T>
__global__ __launch_bounds__(kBlock)
void extract_count_kernel(const T* __restrict__ vol, float threshold, int S, int nb, int2* __restrict__ ws)
{
    __shared__ int2 svq[kWaves];
    const int N = S + 1, cells = N * N * N, b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    unsigned mask = 0;
    if (i < cells) mask = corner_mask<T, false>(vol + (size_t)b * S * S * S, S, threshold, cell_of(i, N), nullptr);
    const int nv = __popcll(__ballot(mask != 0u && mask != 255u)), nq = wave_total(vote2(__popc(quad_flags(mask) & 7u)));
    const int2 n = block_count(make_int2(nv, nq), svq);
    if (threadIdx.x == 0) ws[(size_t)b * nb + blockIdx.x] = n;
}

__global__ __launch_bounds__(kBlock)
void extract_scan_kernel(int2* __restrict__ ws, int nb, int* __restrict__ totals)
{
    __shared__ int2 swave[kWaves];
    const int2 total = scan_totals(ws + (size_t)blockIdx.x * nb, nb, swave);
    if (threadIdx.x == 0) {
        totals[2 * blockIdx.x] = total.x;
        totals[2 * blockIdx.x + 1] = total.y;
    }
}

template <typename T, bool kSmooth>
__global__ __launch_bounds__(kBlock)
void extract_verts_kernel(const T* __restrict__ vol, float threshold, int S, int nb, const int2* __restrict__ ws,
                          const long long* __restrict__ vert_offsets, long long n_verts, int* __restrict__ cellvert,
                          int* __restrict__ q)
{
    __shared__ int sv[kWaves];
    const int N = S + 1, cells = N * N * N, b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const Cell c = cell_of(min(i, cells - 1), N);
    int lev[8];
    unsigned mask = 0;
    if (i < cells) mask = corner_mask<T, kSmooth>(vol + (size_t)b * S * S * S, S, threshold, c, lev);
    const bool active = mask != 0u && mask != 255u;
    const unsigned long long act = __ballot(active);
    const int id = ws[(size_t)b * nb + blockIdx.x].x + block_rank(__popcll(act), lanes_before(act), sv);
    if (i >= cells) return;
    cellvert[(size_t)b * cells + i] = active ? (id | (int)(quad_flags(mask) << kIdBits)) : -1;
    if (!active) return;
    int p[3] = {128, 128, 128};
    if (kSmooth) {
        int sum[3] = {0, 0, 0}, n = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int u = a == 2 ? 0 : a + 1, v = u == 2 ? 0 : u + 1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bu = e >> 1, bv = e & 1;
                const int lo = (bu << (2 - u)) | (bv << (2 - v)), hi = lo | (1 << (2 - a));     // corner numbers of the two ends
                if (((mask >> lo) ^ (mask >> hi)) & 1u) {
                    const int da = lev[lo], db = lev[hi];
                    sum[a] += da + db == 0 ? 128 : (256 * da) / (da + db);                        // 256 * 2^22 = 2^30
                    sum[u] += 256 * bu;
                    sum[v] += 256 * bv;
                    ++n;
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = min(max((2 * sum[a] + n) / (2 * n), 1), 255);          // active: n >= 3
    }
    const long long at = vert_offsets[b] + id;
    if (at < 0 || at >= n_verts) return;                         // offsets that do not belong to this workspace write nothing
    const int cc[3] = {c.c0, c.c1, c.c2};
#pragma unroll
    for (int a = 0; a < 3; ++a) q[3 * at + a] = min(max(256 * cc[a] + 128 + p[a], 0), 256 * S);
}

template <bool kTriangles>
__global__ __launch_bounds__(kBlock)
void extract_quads_kernel(const int* __restrict__ cellvert, int S, int nb, const int2* __restrict__ ws,
                          const long long* __restrict__ quad_offsets, long long n_quads, int* __restrict__ faces)
{
    __shared__ int sq[kWaves];
    const int N = S + 1, cells = N * N * N, b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int* cv = cellvert + (size_t)b * cells;
    const int word = i < cells ? cv[i] : -1;
    const unsigned flags = word < 0 ? 0u : ((unsigned)word >> kIdBits) & 63u;
    const int nq = __popc(flags & 7u);
    const Vote2 quads = vote2(nq);
    int k = ws[(size_t)b * nb + blockIdx.x].y + block_rank(wave_total(quads), lanes_before(quads), sq);
    if (nq == 0) return;
    const int idx[3] = {i / (N * N), i / N % N, i % N};          // c + 1
    const int stride[3] = {N * N, N, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((flags >> a) & 1u)) continue;
        const int u = a == 2 ? 0 : a + 1, v = u == 2 ? 0 : u + 1;
        const long long at = quad_offsets[b] + k;
        ++k;
        if (idx[u] + 1 >= N || idx[v] + 1 >= N || at < 0 || at >= n_quads) continue;             // never for a workspace of this grid
        const int v0 = word & kIdMask, v1 = cv[i + stride[u]] & kIdMask, v2 = cv[i + stride[u] + stride[v]] & kIdMask,
                  v3 = cv[i + stride[v]] & kIdMask;
        const bool keep = (flags >> (3 + a)) & 1u;               // lower end inside: the normal is +a, the ring as it stands
        const int r1 = keep ? v1 : v3, r3 = keep ? v3 : v1;
        if (kTriangles) {
            int2* out = (int2*)(faces + 6 * at);                 // (0,1,2), (0,2,3)
            out[0] = make_int2(v0, r1);
            out[1] = make_int2(v2, v0);
            out[2] = make_int2(v2, r3);
        } else {
            ((int4*)faces)[at] = make_int4(v0, r1, v2, r3);
        }
    }
}

int blocks_per_grid(int S) { return ((S + 1) * (S + 1) * (S + 1) + kBlock - 1) / kBlock; }

// the checks the two entries share; 0 when the arguments are fine
int check_common(const char* who, const void* vol, int vol_is_u8, float threshold, int B, int S, const void* ws, size_t ws_bytes)
{
    if (rn_check_grid_side_pow2(who, S) || rn_check_batch(who, B)) return RN_E_INVALID;
    if (vol_is_u8 != 0 && vol_is_u8 != 1) return rn_set_error(RN_E_INVALID, "%s: vol_is_u8=%d", who, vol_is_u8);
    if (!(threshold == threshold)) return rn_set_error(RN_E_INVALID, "%s: threshold is NaN", who);
    if (B == 0) return RN_OK;
    return rn_check_pointers(who, {vol}) || rn_check_aligned(who, vol, vol_is_u8 ? 1 : 4, "vol") ||
           rn_check_ws(who, ws, ws_bytes, rn_mesh_extract_workspace_bytes(B, S));
}

}  // namespace

extern "C" size_t rn_mesh_extract_workspace_bytes(int B, int S)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B)) return 0;
    return ((size_t)B * blocks_per_grid(S) * sizeof(int2) + 15) / 16 * 16;
}

extern "C" int rn_mesh_extract_count(const void* vol, int vol_is_u8, float threshold, int B, int S, void* workspace,
                                     size_t workspace_bytes, int* totals, void* stream)
{
    if (check_common(__func__, vol, vol_is_u8, threshold, B, S, workspace, workspace_bytes)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(__func__, {totals}) || rn_check_aligned(__func__, totals, 4, "totals")) return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int nb = blocks_per_grid(S);
    const dim3 grid((unsigned)nb, (unsigned)B);
    if (vol_is_u8)
        hipLaunchKernelGGL(extract_count_kernel<unsigned char>, grid, dim3(kBlock), 0, st, (const unsigned char*)vol, threshold, S, nb,
                           (int2*)workspace);
    else
        hipLaunchKernelGGL(extract_count_kernel<float>, grid, dim3(kBlock), 0, st, (const float*)vol, threshold, S, nb, (int2*)workspace);
    hipLaunchKernelGGL(extract_scan_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, (int2*)workspace, nb, totals);
    return rn_check_launch(__func__);
}

extern "C" int rn_mesh_extract_emit(const void* vol, int vol_is_u8, float threshold, int B, int S, int mode, int triangles,
                                    const void* workspace, size_t workspace_bytes, const long long* vert_offsets,
                                    const long long* quad_offsets, long long n_verts, long long n_quads, int* cellvert, int* q,
                                    int* faces, void* stream)
{
    const char* who = __func__;
    if (check_common(who, vol, vol_is_u8, threshold, B, S, workspace, workspace_bytes)) return RN_E_INVALID;
    if (mode != RN_EXTRACT_BLOCKY && mode != RN_EXTRACT_SMOOTH)
        return rn_set_error(RN_E_INVALID, "%s: mode=%d (0 blocky, 1 smooth)", who, mode);
    if (triangles != 0 && triangles != 1) return rn_set_error(RN_E_INVALID, "%s: triangles=%d", who, triangles);
    if (n_verts < 0 || n_quads < 0) return rn_set_error(RN_E_INVALID, "%s: n_verts=%lld n_quads=%lld", who, n_verts, n_quads);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(who, {vert_offsets, quad_offsets, cellvert}) || (n_verts > 0 && rn_check_pointers(who, {q})) ||
        (n_quads > 0 && rn_check_pointers(who, {faces})) ||
        rn_check_aligned(who, vert_offsets, 8, "vert_offsets") || rn_check_aligned(who, quad_offsets, 8, "quad_offsets") ||
        rn_check_aligned(who, cellvert, 4, "cellvert") || rn_check_aligned(who, q, 4, "q") || rn_check_aligned(who, faces, 16, "faces"))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int nb = blocks_per_grid(S);
    const dim3 grid((unsigned)nb, (unsigned)B), block(kBlock);
    const int2* ws = (const int2*)workspace;
#define RN_EXTRACT_VERTS(T, SMOOTH)                                                                                              \
    hipLaunchKernelGGL((extract_verts_kernel<T, SMOOTH>), grid, block, 0, st, (const T*)vol, threshold, S, nb, ws, vert_offsets, \
                       n_verts, cellvert, q)
    if (vol_is_u8) {
        if (mode == RN_EXTRACT_SMOOTH) RN_EXTRACT_VERTS(unsigned char, true);
        else RN_EXTRACT_VERTS(unsigned char, false);
    } else {
        if (mode == RN_EXTRACT_SMOOTH) RN_EXTRACT_VERTS(float, true);
        else RN_EXTRACT_VERTS(float, false);
    }
#undef RN_EXTRACT_VERTS
    if (n_quads > 0) {
        if (triangles)
            hipLaunchKernelGGL(extract_quads_kernel<true>, grid, block, 0, st, cellvert, S, nb, ws, quad_offsets, n_quads, faces);
        else
            hipLaunchKernelGGL(extract_quads_kernel<false>, grid, block, 0, st, cellvert, S, nb, ws, quad_offsets, n_quads, faces);
    }
    return rn_check_launch(who);
}
