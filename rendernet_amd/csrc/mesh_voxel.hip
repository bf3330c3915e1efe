// Mesh voxeliser: the occupancy grid of a triangle mesh on the 1/256-voxel lattice (gfx950), the mesh input of the renderer, the
// ray casters and the synthetic training feeds.  The grid is a deterministic INTEGER function of the lattice vertices; the two
// rules, their tie decisions, the clamps and the bounds that keep every intermediate inside 64 bits are stated in
// include/rendernet_hip.h (rn_mesh_voxelize), the NumPy twin is tests/mesh_voxel_ref.py.  No float appears in this file.
//
// Bounds in short (the header derives them): coordinates are clamped to [0, 256 S] <= 2^15 at S = 128, differences |d| <= 2^15,
// edge functions and areas |E_k|, |A| <= 2^31 (one bit too many for int: 64-bit), crossing depth 0 <= N <= 2^46, surface
// normals |n_i| <= 2^31 and plane sums below 2^48.  Everything that is a product of two differences is long long.
//
// Accumulation: a solid crossing flips bits k .. S-1 of its column with atomicXor on at most S/32 words, a surface overlap sets
// one bit with atomicOr, both straight into the global work masks.  XOR and OR commute and associate, so the masks hold the same
// bits whatever order the atomics arrive in: two calls give identical bytes without any ordering between triangles.
//
//   mesh_solid_kernel<false> / mesh_surface_kernel<false>   small triangles (at most a few dozen candidates): one per lane
//   mesh_solid_kernel<true>  / mesh_surface_kernel<true>    large triangles: one per wave, the lanes stride the candidates; a
//                        short list is launched in slices (gridDim.y waves per triangle, striding together) until about
//                        kLargeWaves waves are in flight: twelve triangles that fill a 128^3 grid are 32 000 candidates each
//   mesh_expand_kernel   ORs the two masks; a thread writes 16 voxels as bytes with one 128-bit store (the nibble-spreading
//                        multiply of voxel_shapes.hip) and every second thread the combined 32-bit word
#include "voxel_common.h"
#include "rn_checks.h"

namespace {

typedef long long i64;
#ifndef RN_MESH_LARGE_WAVES
#define RN_MESH_LARGE_WAVES 2048                                 // 256 CUs x 8 waves; 1 = one wave per large triangle (the A/B's other leg)
#endif
constexpr int kLargeWaves = RN_MESH_LARGE_WAVES, kMaxSlices = 64;

struct Tri { int p[3][3]; };                                     // [vertex][array axis], clamped to [0, 256 S]

__device__ __forceinline__ Tri load_tri(const int* __restrict__ verts, int V, const int* __restrict__ tris, int t, int S)
{
    Tri r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = min(max(tris[3 * (size_t)t + k], 0), V - 1);           // ops checks the range; a stray index stays inside verts
#pragma unroll
        for (int a = 0; a < 3; ++a) r.p[k][a] = min(max(verts[3 * (size_t)v + a], 0), 256 * S);
    }
    return r;
}

// voxels whose centre 256 k + 128 lies in [lo, hi], clipped to the grid; 0 <= lo <= hi <= 256 S
__device__ __forceinline__ void centre_range(int lo, int hi, int S, int& first, int& count)
{
    first = max((lo + 127) >> 8, 0);                             // ceil((lo - 128) / 256), arithmetic shift = floor
    const int last = min((hi - 128) >> 8, S - 1);
    count = max(last - first + 1, 0);
}

// voxels whose closed cell [256 k, 256 (k + 1)] meets [lo, hi], clipped to the grid
__device__ __forceinline__ void cell_range(int lo, int hi, int S, int& first, int& count)
{
    first = max(((lo + 255) >> 8) - 1, 0);
    const int last = min(hi >> 8, S - 1);
    count = max(last - first + 1, 0);
}

struct SolidTri {                                                // oriented so that A > 0
    int u[3], v[3], w[3];
    i64 A;
    int i0, ni, j0, nj;
};

__device__ __forceinline__ bool solid_setup(const Tri& t, int S, SolidTri& s)
{
    int k1 = 1, k2 = 2;
    i64 A = (i64)(t.p[1][0] - t.p[0][0]) * (t.p[2][1] - t.p[0][1]) - (i64)(t.p[1][1] - t.p[0][1]) * (t.p[2][0] - t.p[0][0]);
    if (A == 0) return false;
    if (A < 0) { k1 = 2; k2 = 1; A = -A; }
    const int order[3] = {0, k1, k2};
#pragma unroll
    for (int k = 0; k < 3; ++k) { s.u[k] = t.p[order[k]][0]; s.v[k] = t.p[order[k]][1]; s.w[k] = t.p[order[k]][2]; }
    s.A = A;
    centre_range(min(min(s.u[0], s.u[1]), s.u[2]), max(max(s.u[0], s.u[1]), s.u[2]), S, s.i0, s.ni);
    centre_range(min(min(s.v[0], s.v[1]), s.v[2]), max(max(s.v[0], s.v[1]), s.v[2]), S, s.j0, s.nj);
    return s.ni > 0 && s.nj > 0;
}

// column (i, j), 0 <= i, j < S: flips bits k .. S-1 when the centre is inside the projected triangle
__device__ __forceinline__ void solid_column(const SolidTri& s, int i, int j, int S, unsigned* __restrict__ mask)
{
    const int cu = 256 * i + 128, cv = 256 * j + 128;
    i64 E[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int n = k == 2 ? 0 : k + 1;
        const int du = s.u[n] - s.u[k], dv = s.v[n] - s.v[k];
        E[k] = (i64)du * (cv - s.v[k]) - (i64)dv * (cu - s.u[k]);
        const bool owns = dv > 0 || (dv == 0 && du < 0);
        if (!(E[k] > 0 || (E[k] == 0 && owns))) return;
    }
    const i64 N = E[0] * s.w[2] + E[1] * s.w[0] + E[2] * s.w[1];
    i64 k = floor_div(N - 128 * s.A, 256 * s.A) + 1;             // first voxel whose centre is strictly behind the crossing
    k = k < 0 ? 0 : k;
    if (k >= S) return;
    const int words = S >> 5, kw = (int)k >> 5;
    unsigned* col = mask + (size_t)(i * S + j) * words;          // (i S + j) S bits: S/32 whole words
    atomicXor(col + kw, 0xffffffffu << ((int)k & 31));
    for (int w = kw + 1; w < words; ++w) atomicXor(col + w, 0xffffffffu);
}

struct SurfTri {
    int p[3][3];
    i64 n[3];
    int f[3], c[3];                                              // first candidate voxel and count per axis
};

__device__ __forceinline__ bool surf_setup(const Tri& t, int S, SurfTri& s)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) s.p[k][a] = t.p[k][a];
    const int e0[3] = {t.p[1][0] - t.p[0][0], t.p[1][1] - t.p[0][1], t.p[1][2] - t.p[0][2]};
    const int e1[3] = {t.p[2][0] - t.p[1][0], t.p[2][1] - t.p[1][1], t.p[2][2] - t.p[1][2]};
    s.n[0] = (i64)e0[1] * e1[2] - (i64)e0[2] * e1[1];
    s.n[1] = (i64)e0[2] * e1[0] - (i64)e0[0] * e1[2];
    s.n[2] = (i64)e0[0] * e1[1] - (i64)e0[1] * e1[0];
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cell_range(min(min(t.p[0][a], t.p[1][a]), t.p[2][a]), max(max(t.p[0][a], t.p[1][a]), t.p[2][a]), S, s.f[a], s.c[a]);
        any = any && s.c[a] > 0;
    }
    return any;
}

__device__ __forceinline__ i64 iabs(i64 x) { return x < 0 ? -x : x; }

// voxel (x0, x1, x2) inside the grid: sets its bit when the closed cube meets the closed triangle (plane + nine edge axes; the
// three cube axes are the candidate range)
__device__ __forceinline__ void surf_voxel(const SurfTri& s, int x0, int x1, int x2, int S, unsigned* __restrict__ mask)
{
    const int c[3] = {256 * x0 + 128, 256 * x1 + 128, 256 * x2 + 128};
    int q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) q[k][a] = s.p[k][a] - c[a];
    const i64 d = s.n[0] * q[0][0] + s.n[1] * q[0][1] + s.n[2] * q[0][2];
    if (iabs(d) > 128 * (iabs(s.n[0]) + iabs(s.n[1]) + iabs(s.n[2]))) return;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int n = e == 2 ? 0 : e + 1;
        const int ed[3] = {q[n][0] - q[e][0], q[n][1] - q[e][1], q[n][2] - q[e][2]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // a = ed x unit_j: a[j] = 0, a[j1] = ed[j2], a[j2] = -ed[j1] with (j, j1, j2) cyclic
            const int j1 = j == 2 ? 0 : j + 1, j2 = j1 == 2 ? 0 : j1 + 1;
            const int a1 = ed[j2], a2 = -ed[j1];
            i64 lo = (i64)a1 * q[0][j1] + (i64)a2 * q[0][j2], hi = lo;
#pragma unroll
            for (int k = 1; k < 3; ++k) {
                const i64 v = (i64)a1 * q[k][j1] + (i64)a2 * q[k][j2];
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            const i64 r = 128 * (iabs((i64)a1) + iabs((i64)a2));
            if (lo > r || hi < -r) return;
        }
    }
    const unsigned i = (unsigned)((x0 * S + x1) * S + x2);
    atomicOr(mask + (i >> 5), 1u << (i & 31));
}

template <bool kLarge>
__global__ __launch_bounds__(kBlock)
void mesh_solid_kernel(const int* __restrict__ verts, int V, const int* __restrict__ tris, int T, const int* __restrict__ list,
                       int n, unsigned* __restrict__ mask, int S)
{
    const int gid = blockIdx.x * kBlock + threadIdx.x;
    const int item = kLarge ? gid / kWave : gid;
    if (item >= n) return;
    SolidTri s;
    if (!solid_setup(load_tri(verts, V, tris, min(max(list[item], 0), T - 1), S), S, s)) return;
    const int total = s.ni * s.nj;                               // <= 128 * 128
    for (int c = kLarge ? gid % kWave + kWave * blockIdx.y : 0; c < total; c += kLarge ? kWave * gridDim.y : 1)
        solid_column(s, s.i0 + c / s.nj, s.j0 + c % s.nj, S, mask);
}

template <bool kLarge>
__global__ __launch_bounds__(kBlock)
void mesh_surface_kernel(const int* __restrict__ verts, int V, const int* __restrict__ tris, int T, const int* __restrict__ list,
                         int n, unsigned* __restrict__ mask, int S)
{
    const int gid = blockIdx.x * kBlock + threadIdx.x;
    const int item = kLarge ? gid / kWave : gid;
    if (item >= n) return;
    SurfTri s;
    if (!surf_setup(load_tri(verts, V, tris, min(max(list[item], 0), T - 1), S), S, s)) return;
    const int plane = s.c[1] * s.c[2], total = s.c[0] * plane;   // <= 128^3 = 2^21
    for (int c = kLarge ? gid % kWave + kWave * blockIdx.y : 0; c < total; c += kLarge ? kWave * gridDim.y : 1) {
        const int r = c % plane;
        surf_voxel(s, s.f[0] + c / plane, s.f[1] + r / s.c[2], s.f[2] + r % s.c[2], S, mask);
    }
}

// the work masks are cleared by a kernel, not a memset node: a captured graph keeps kernels in order (see word_kernel, conv_wino_bf3.hip)
__global__ __launch_bounds__(kBlock)
void mesh_clear_kernel(uint4* __restrict__ ws) { ws[blockIdx.x * kBlock + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u); }

// thread t: voxels 16 t .. 16 t + 15, the low or high half of word t >> 1
__global__ __launch_bounds__(kBlock)
void mesh_expand_kernel(const unsigned* __restrict__ solid, const unsigned* __restrict__ surf, unsigned* __restrict__ bits,
                        uint4* __restrict__ vox)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;             // S^3 / 16 threads, whole blocks at every S
    const unsigned word = solid[t >> 1] | surf[t >> 1];
    if ((t & 1) == 0) bits[t >> 1] = word;
    const unsigned occ = (t & 1) ? word >> 16 : word & 0xffffu;
    // four bits -> four bytes of 0 / 1: bit k lands on bit 8k through the term 2^(7k); no two terms meet, so nothing carries
    uint4 o;
    o.x = ((occ & 15u) * 0x00204081u) & 0x01010101u;
    o.y = (((occ >> 4) & 15u) * 0x00204081u) & 0x01010101u;
    o.z = (((occ >> 8) & 15u) * 0x00204081u) & 0x01010101u;
    o.w = (((occ >> 12) & 15u) * 0x00204081u) & 0x01010101u;
    vox[t] = o;
}

}  // namespace

extern "C" int rn_mesh_voxelize(const int* verts, int V, const int* tris, int T,
                                const int* small_solid, int n_ss, const int* large_solid, int n_ls,
                                const int* small_surf, int n_sf, const int* large_surf, int n_lf,
                                unsigned* ws_bits, unsigned* bits, unsigned char* vox, int S, int mode, void* stream)
{
    if (rn_check_grid_side_pow2(__func__, S)) return RN_E_INVALID;
    if (mode < RN_MESH_SOLID || mode > RN_MESH_BOTH)
        return rn_set_error(RN_E_INVALID, "rn_mesh_voxelize: mode=%d (1 solid, 2 surface, 3 both)", mode);
    if (V < 0 || T < 0 || (T > 0 && V == 0)) return rn_set_error(RN_E_INVALID, "rn_mesh_voxelize: V=%d T=%d", V, T);
    if (n_ss < 0 || n_ls < 0 || n_sf < 0 || n_lf < 0 || (T == 0 && (n_ss | n_ls | n_sf | n_lf) != 0))
        return rn_set_error(RN_E_INVALID, "rn_mesh_voxelize: list lengths %d %d %d %d for T=%d", n_ss, n_ls, n_sf, n_lf, T);
    if (n_ls > (1 << 24) || n_lf > (1 << 24))
        return rn_set_error(RN_E_INVALID, "rn_mesh_voxelize: %d / %d large triangles (at most 2^24 per list)", n_ls, n_lf);
    if (rn_check_pointers(__func__, {ws_bits, bits, vox}) || (T > 0 && rn_check_pointers(__func__, {verts, tris})) ||
        (n_ss > 0 && rn_check_pointers(__func__, {small_solid})) || (n_ls > 0 && rn_check_pointers(__func__, {large_solid})) ||
        (n_sf > 0 && rn_check_pointers(__func__, {small_surf})) || (n_lf > 0 && rn_check_pointers(__func__, {large_surf})) ||
        rn_check_aligned(__func__, ws_bits, 16, "ws_bits") || rn_check_aligned(__func__, bits, 16, "bits") ||
        rn_check_aligned(__func__, vox, 16, "vox"))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t words = (size_t)S * S * S / 32;
    unsigned* solid = ws_bits;
    unsigned* surf = ws_bits + words;
    static_assert(2 * (32 * 32 * 32 / 32) / 4 % kBlock == 0, "whole blocks at every size");
    hipLaunchKernelGGL(mesh_clear_kernel, dim3((unsigned)(2 * words / 4 / kBlock)), dim3(kBlock), 0, st, (uint4*)ws_bits);
    auto blocks = [](long long threads) { return dim3((unsigned)((threads + kBlock - 1) / kBlock)); };
    auto sliced = [&](int n) { return dim3(blocks((long long)n * kWave).x, (unsigned)min(max(kLargeWaves / n, 1), kMaxSlices)); };
    if (mode & RN_MESH_SOLID) {
        if (n_ss > 0)
            hipLaunchKernelGGL(mesh_solid_kernel<false>, blocks(n_ss), dim3(kBlock), 0, st, verts, V, tris, T, small_solid, n_ss, solid, S);
        if (n_ls > 0)
            hipLaunchKernelGGL(mesh_solid_kernel<true>, sliced(n_ls), dim3(kBlock), 0, st, verts, V, tris, T,
                               large_solid, n_ls, solid, S);
    }
    if (mode & RN_MESH_SURFACE) {
        if (n_sf > 0)
            hipLaunchKernelGGL(mesh_surface_kernel<false>, blocks(n_sf), dim3(kBlock), 0, st, verts, V, tris, T, small_surf, n_sf, surf, S);
        if (n_lf > 0)
            hipLaunchKernelGGL(mesh_surface_kernel<true>, sliced(n_lf), dim3(kBlock), 0, st, verts, V, tris, T,
                               large_surf, n_lf, surf, S);
    }
    static_assert(32 * 32 * 32 / 16 % kBlock == 0, "whole blocks at every size");
    hipLaunchKernelGGL(mesh_expand_kernel, dim3((unsigned)(words * 2 / kBlock)), dim3(kBlock), 0, st, solid, surf, bits, (uint4*)vox);
    return rn_check_launch("rn_mesh_voxelize");
}
