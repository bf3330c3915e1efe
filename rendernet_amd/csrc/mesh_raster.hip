// Mesh rasteriser: the normal map of a triangle mesh under the ray caster's camera, as 8-bit frames (gfx950), the target of the
// synthetic mesh feed and the picture the demo writes beside its voxel views.  Visibility and depth are INTEGER functions of the
// lattice vertices and the integer camera; geometry, tie rule, clamps, bounds and the encoding are stated in
// include/rendernet_hip.h (rn_mesh_rasterize), the NumPy twin is tests/mesh_raster_ref.py.  Built with -ffp-contract=off: the
// camera (float64) and the normal bytes (float32) round every operation on its own, as the twin reads them.
//
// Bounds in short (the header derives them): projected X, Y are clamped to +-2^20 and Z to +-2^17, pixel centres lie in [0, 2^19),
// so edge functions and areas stay below 2^43 and the depth numerator below 3 * 2^60: everything that is a product is long long.
//
//   mesh_camera_kernel    thread b < B: float64 inverse of item b's M_inv -> cam [b] (three affine rows, 2^20 fixed point).  The same
//                         launch fills the visibility buffer with the miss key (every thread strides it): the raster launch's
//                         atomics need it initialised by an EARLIER launch, there is no ordering inside one.
//   mesh_raster_kernel    lane = (item, triangle): project, area, cull, box.  A box of at most kLaneBox pixels is walked by its
//                         lane; larger ones are taken over by the whole wave one after another (ballot, leader = lowest lane, every
//                         lane repeats the leader's setup and strides its pixels), so no lane serialises a large triangle.  A
//                         fragment is one 64-bit atomicMin of (depth << 32 | triangle): a minimum commutes, the picture does not
//                         depend on arrival order or on the split.
//   mesh_resolve_kernel   thread = pixel: key -> triangle id, depth and the normal bytes (the winner's setup again, E_k / A weights).
//   mesh_vnormal_kernel   lane = triangle of the concatenated set: its lattice cross product into the three vertices' int64 sums
//                         with integer atomicAdd (commutes: identical bits every run).  Once per mesh set, not per batch.
//   mesh_colour_kernel    thread = pixel: triangle id -> a face colour, or the three vertex colours weighted E_k / A in integers
//                         (rn_mesh_colour_from_ids: the resolve's setup once more, no float anywhere).  A gather.
//   mesh_face_voxels_kernel  thread = face of a surface net: the cells of its first three vertices name the sample edge it was
//                         emitted for; the inside end's flat id (rn_mesh_face_voxels).  A gather.
#include "voxel_common.h"
#include "rn_checks.h"
#include "mesh_project.h"

namespace {

#ifndef RN_RASTER_LANE_BOX
#define RN_RASTER_LANE_BOX 32                                    // the one threshold: a larger pixel box goes to the whole wave
#endif
constexpr int kLaneBox = RN_RASTER_LANE_BOX;
constexpr u64 kMiss = ~0ull;

struct Meshes {                                                  // the concatenated set
    const int* verts; i64 V;
    const int* tris; i64 T;
    const i64* vert_offsets; const i64* tri_offsets; int M;     // [M+1] each
};

// the slice of mesh m, every offset clamped into its array: v0 <= v1 <= V, t0 <= t1 <= T
__device__ __forceinline__ void mesh_slice(const Meshes& ms, int m, i64& v0, i64& v1, i64& t0, i64& t1)
{
    m = min(max(m, 0), ms.M - 1);
    v0 = clampi(ms.vert_offsets[m], 0, ms.V);
    v1 = clampi(ms.vert_offsets[m + 1], v0, ms.V);
    t0 = clampi(ms.tri_offsets[m], 0, ms.T);
    t1 = clampi(ms.tri_offsets[m + 1], t0, ms.T);
}

// lattice vertices of triangle t0 + t (t < t1 - t0, v1 > v0), coordinates clamped to [0, 256 S]; p[k][a]: vertex k, array axis a
__device__ __forceinline__ void load_tri(const Meshes& ms, i64 v0, i64 v1, i64 tg, int S, int p[3][3], i64 vid[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const i64 v = v0 + clampi((i64)ms.tris[3 * tg + k], 0, v1 - v0 - 1);       // a stray index stays inside its mesh
        vid[k] = v;
#pragma unroll
        for (int a = 0; a < 3; ++a) p[k][a] = min(max(ms.verts[3 * v + a], 0), 256 * S);
    }
}

__device__ __forceinline__ void cross_of(const int p[3][3], i64 n[3])               // (p1 - p0) x (p2 - p1), array-axis order
{
    const i64 e0[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const i64 e1[3] = {p[2][0] - p[1][0], p[2][1] - p[1][1], p[2][2] - p[1][2]};
    n[0] = e0[1] * e1[2] - e0[2] * e1[1];
    n[1] = e0[2] * e1[0] - e0[0] * e1[2];
    n[2] = e0[0] * e1[1] - e0[1] * e1[0];
}

struct ScreenTri {                                               // wound to A > 0: order[k] = the input vertex at position k
    i64 X[3], Y[3], Z[3], A;
    int order[3];
    bool back;                                                   // the viewer sees the inward side (cull "none" only)
    int c0, c1, r0, r1;                                          // inclusive pixel box inside the window; empty when c1 < c0 or r1 < r0
};

// project, area, cull, box.  false: the triangle draws nothing.
__device__ __forceinline__ bool screen_setup(const int p[3][3], const i64* __restrict__ cam, int cull_back, int low_x,
                                             int row0, int col0, int ph, int pw, ScreenTri& s)
{
    i64 n[3];
    cross_of(p, n);
    if ((n[0] | n[1] | n[2]) == 0) return false;                 // no lattice normal: nothing to shade (mesh.prepare drops these too)
    i64 P[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) P[k][r] = project_row(cam, r, p[k][0], p[k][1], p[k][2]);
    i64 A = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[1][1] - P[0][1]) * (P[2][0] - P[0][0]);
    if (A == 0) return false;
    const bool front = low_x ? A > 0 : A < 0;
    if (cull_back && !front) return false;
    s.back = !front;
    s.order[0] = 0;
    s.order[1] = A < 0 ? 2 : 1;
    s.order[2] = A < 0 ? 1 : 2;
    s.A = A < 0 ? -A : A;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = k == 0 ? 0 : (A < 0 ? 3 - k : k);
        s.X[k] = P[o][0]; s.Y[k] = P[o][1]; s.Z[k] = P[o][2];
    }
    const i64 xlo = min(min(s.X[0], s.X[1]), s.X[2]), xhi = max(max(s.X[0], s.X[1]), s.X[2]);
    const i64 ylo = min(min(s.Y[0], s.Y[1]), s.Y[2]), yhi = max(max(s.Y[0], s.Y[1]), s.Y[2]);
    // pixels whose centre 256 k + 128 lies in [lo, hi]: ceil((lo - 128) / 256) .. floor((hi - 128) / 256), shifts floor towards -inf
    s.c0 = (int)max((xlo + 127) >> 8, (i64)col0);
    s.c1 = (int)min((xhi - 128) >> 8, (i64)col0 + pw - 1);
    s.r0 = (int)max((ylo + 127) >> 8, (i64)row0);
    s.r1 = (int)min((yhi - 128) >> 8, (i64)row0 + ph - 1);
    return s.c1 >= s.c0 && s.r1 >= s.r0;
}

// pixel (r, c) of the full frame against a wound triangle: inside -> E[3]
__device__ __forceinline__ bool edge_functions(const ScreenTri& s, int r, int c, i64 E[3])
{
    const i64 cu = 256 * (i64)c + 128, cv = 256 * (i64)r + 128;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int n = k == 2 ? 0 : k + 1;
        const i64 du = s.X[n] - s.X[k], dv = s.Y[n] - s.Y[k];
        E[k] = du * (cv - s.Y[k]) - dv * (cu - s.X[k]);
        const bool owns = dv > 0 || (dv == 0 && du < 0);
        in = in && (E[k] > 0 || (E[k] == 0 && owns));
    }
    return in;
}

__device__ __forceinline__ void fragment(const ScreenTri& s, int r, int c, int t, int N, u64* __restrict__ keys_b,
                                         int row0, int col0, int pw)
{
    i64 E[3];
    if (!edge_functions(s, r, c, E)) return;
    const i64 d = floor_div(E[0] * s.Z[2] + E[1] * s.Z[0] + E[2] * s.Z[1], s.A);
    if (d < 0 || d > 256 * (i64)N) return;                       // the caster's ray ends
    atomicMin(keys_b + (size_t)(r - row0) * pw + (c - col0), ((u64)d << 32) | (u64)(unsigned)t);
}

// ---- camera ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ i64 to_fixed(double v, double limit)
{
    const double s = rint(v * 1048576.0);
    if (!(s == s)) return 0;                                     // NaN
    return (i64)fmin(fmax(s, -limit), limit);
}

__global__ __launch_bounds__(kBlock)
void mesh_camera_kernel(const float* __restrict__ m_inv, i64* __restrict__ cam, int B, int N, int f, int low_x,
                        u64* __restrict__ keys, size_t n_keys)
{
    const size_t gid = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (keys)
        for (size_t i = gid; i < n_keys; i += (size_t)gridDim.x * kBlock) keys[i] = kMiss;
    if (gid >= (size_t)B) return;
    const float* Mf = m_inv + gid * 12;
    double m[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[i][j] = (double)Mf[4 * i + j];
    // F = inverse of [M; 0 0 0 1]: adjugate of the 3x3 part over its determinant, translation -L^-1 t
    double c[3][3];
    c[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    c[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2];
    c[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    c[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    c[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
    c[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    c[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    c[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
    c[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    const double det = (m[0][0] * c[0][0] + m[0][1] * c[1][0]) + m[0][2] * c[2][0];
    double F[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) F[i][j] = c[i][j] / det;
        F[i][3] = -((F[i][0] * m[0][3] + F[i][1] * m[1][3]) + F[i][2] * m[2][3]);
    }
    const bool ok = det != 0.0 && det == det && fabs(det) <= 1.7e308;
    // rows 256 X, 256 Y, 256 D as affine functions of (q0, q1, q2); source (x, y, z) = (q2, q1, q0) / 256 - 0.5
    const double fd = (double)f, Nd = (double)N;
    const int src[3] = {2, 1, 0};                                // the camera row each output row reads: X <- zc, Y <- yc, D <- xc
    const double sign[3] = {1.0, -1.0, low_x ? 1.0 : -1.0};
    const double scale[3] = {fd, fd, 1.0};
    i64* out = cam + gid * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double* Fr = F[src[r]];
        const double half = 0.5 * ((Fr[0] + Fr[1]) + Fr[2]);
        // camera coordinate of the vertex: (Fr . (q2, q1, q0)) / 256 + (Fr[3] - half)
        const double offs = Fr[3] - half;
        const double b = sign[r] > 0.0 ? offs + 0.5 : (Nd - 0.5) - offs;            // X = f (zc + 0.5), Y = f (N - 0.5 - yc), D likewise
        out[4 * r + 0] = ok ? to_fixed(sign[r] * scale[r] * Fr[2], 1099511627776.0) : 0;
        out[4 * r + 1] = ok ? to_fixed(sign[r] * scale[r] * Fr[1], 1099511627776.0) : 0;
        out[4 * r + 2] = ok ? to_fixed(sign[r] * scale[r] * Fr[0], 1099511627776.0) : 0;
        out[4 * r + 3] = ok ? to_fixed(256.0 * scale[r] * b, 1152921504606846976.0) : 0;
    }
}

// ---- raster ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void mesh_raster_kernel(Meshes ms, const int* __restrict__ mesh_of_item, const i64* __restrict__ cam, u64* __restrict__ keys,
                        int S, int N, int row0, int col0, int ph, int pw, int cull_back, int low_x)
{
    const int b = blockIdx.y;
    const i64 t = (i64)blockIdx.x * kBlock + threadIdx.x;       // every lane stays to the end: the wave path below is collective
    i64 v0, v1, t0, t1;
    mesh_slice(ms, mesh_of_item[b], v0, v1, t0, t1);
    const i64* camb = cam + (size_t)b * 12;
    u64* keys_b = keys + (size_t)b * ph * pw;
    const bool have = t < t1 - t0 && v1 > v0;

    ScreenTri s;
    bool draws = false;
    if (have) {
        int p[3][3];
        i64 vid[3];
        load_tri(ms, v0, v1, t0 + t, S, p, vid);
        draws = screen_setup(p, camb, cull_back, low_x, row0, col0, ph, pw, s);
    }
    const int bw = draws ? s.c1 - s.c0 + 1 : 0, bh = draws ? s.r1 - s.r0 + 1 : 0;
    const i64 box = (i64)bw * bh;                                // <= 2048^2
    if (draws && box <= kLaneBox)
        for (int i = 0; i < (int)box; ++i) fragment(s, s.r0 + i / bw, s.c0 + i % bw, (int)t, N, keys_b, row0, col0, pw);

    u64 pending = __ballot(draws && box > kLaneBox);
    const int lane = threadIdx.x & (kWave - 1);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        const i64 tl = t - lane + leader;                        // the leader's triangle: lanes of a wave hold consecutive ones
        int p[3][3];
        i64 vid[3];
        ScreenTri w;
        load_tri(ms, v0, v1, t0 + tl, S, p, vid);
        if (!screen_setup(p, camb, cull_back, low_x, row0, col0, ph, pw, w)) continue;    // cannot happen: the leader drew
        const int ww = w.c1 - w.c0 + 1;
        const i64 total = (i64)ww * (w.r1 - w.r0 + 1);
        for (i64 i = lane; i < total; i += kWave)
            fragment(w, w.r0 + (int)(i / ww), w.c0 + (int)(i % ww), (int)tl, N, keys_b, row0, col0, pw);
    }
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void normalise3(float v[3])
{
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = v[a] / len;
}

__global__ __launch_bounds__(kBlock)
void mesh_resolve_kernel(Meshes ms, const int* __restrict__ mesh_of_item, const i64* __restrict__ cam,
                         const float* __restrict__ m_inv, const i64* __restrict__ vnorm, const u64* __restrict__ keys,
                         unsigned char* __restrict__ out_u8, int* __restrict__ tri_id, int* __restrict__ depth,
                         int S, int row0, int col0, int ph, int pw, int low_x)
{
    const int b = blockIdx.y;
    const int px = blockIdx.x * kBlock + threadIdx.x;
    if (px >= ph * pw) return;
    const size_t o = (size_t)b * ph * pw + px;
    const u64 key = keys[o];
    i64 v0, v1, t0, t1;
    mesh_slice(ms, mesh_of_item[b], v0, v1, t0, t1);
    const i64 t = (i64)(key & 0xffffffffull);
    int id = -1, d = -1;
    unsigned char rgb[3] = {0, 0, 0};
    if (key != kMiss && t < t1 - t0 && v1 > v0) {
        id = (int)t;
        d = (int)(key >> 32);
        int p[3][3];
        i64 vid[3];
        ScreenTri s;
        load_tri(ms, v0, v1, t0 + t, S, p, vid);
        // the winner's setup again, culling off: `back` says which side the viewer sees
        const bool drew = screen_setup(p, cam + (size_t)b * 12, 0, low_x, row0, col0, ph, pw, s);
        i64 nf[3];
        cross_of(p, nf);
        const float flip = (drew && s.back) ? -1.0f : 1.0f;
        float face[3] = {flip * (float)nf[0], flip * (float)nf[1], flip * (float)nf[2]};
        float n[3] = {face[0], face[1], face[2]};
        if (vnorm && drew) {
            i64 E[3];
            edge_functions(s, row0 + px / pw, col0 + px % pw, E);
            // vertex at wound position k carries E_(k+1): E_0 -> position 2, E_1 -> position 0, E_2 -> position 1, as in the depth
            const float Af = (float)s.A;
            const float w[3] = {(float)E[1] / Af, (float)E[2] / Af, (float)E[0] / Af};
            float acc[3] = {0.0f, 0.0f, 0.0f};
            bool zero = false;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const i64* vs = vnorm + 3 * vid[s.order[k]];
                zero = zero || (vs[0] | vs[1] | vs[2]) == 0;
                float vn[3] = {(float)vs[0], (float)vs[1], (float)vs[2]};
                normalise3(vn);
#pragma unroll
                for (int a = 0; a < 3; ++a) acc[a] = acc[a] + w[k] * vn[a];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[a] = flip * acc[a];
            const float dot = (acc[0] * face[0] + acc[1] * face[1]) + acc[2] * face[2];
            if (!zero && dot > 0.0f) { n[0] = acc[0]; n[1] = acc[1]; n[2] = acc[2]; }
        }
        // n is in array-axis order [zs][ys][xs]; the caster's n_src is (x, y, z)
        const float ns[3] = {n[2], n[1], n[0]};
        const float* M = m_inv + (size_t)b * 12;
        float c[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = (M[j] * ns[0] + M[4 + j] * ns[1]) + M[8 + j] * ns[2];
        const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        const float comp[3] = {c[2] / len, c[1] / len, (low_x ? -c[0] : c[0]) / len};   // right, up, towards
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = 255.0f * (0.5f + 0.5f * comp[j]);
            rgb[j] = (v >= 0.0f && v <= 255.0f) ? (unsigned char)(int)rintf(v) : (unsigned char)128;   // a singular M: no direction
        }
    }
    out_u8[o * 3 + 0] = rgb[0];
    out_u8[o * 3 + 1] = rgb[1];
    out_u8[o * 3 + 2] = rgb[2];
    if (tri_id) tri_id[o] = id;
    if (depth) depth[o] = d;
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void mesh_clear_i64_kernel(i64* __restrict__ dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = 0;
}

__global__ __launch_bounds__(kBlock)
void mesh_vnormal_kernel(Meshes ms, int S, i64* __restrict__ vnorm)
{
    const i64 tg = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (tg >= ms.T) return;
    int lo = 0, hi = ms.M - 1;                                   // the mesh that owns triangle tg: last m with tri_offsets[m] <= tg
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (clampi(ms.tri_offsets[mid], 0, ms.T) <= tg) lo = mid; else hi = mid - 1;
    }
    i64 v0, v1, t0, t1;
    mesh_slice(ms, lo, v0, v1, t0, t1);
    if (tg < t0 || tg >= t1 || v1 <= v0) return;
    int p[3][3];
    i64 vid[3], n[3];
    load_tri(ms, v0, v1, tg, S, p, vid);
    cross_of(p, n);
    if ((n[0] | n[1] | n[2]) == 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicAdd((u64*)(vnorm + 3 * vid[k] + a), (u64)n[a]);     // two's complement: the signed sum
}

// ---- colour resolve -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void mesh_colour_kernel(Meshes ms, const int* __restrict__ mesh_of_item, const i64* __restrict__ cam, const int* __restrict__ tri_id,
                        const unsigned char* __restrict__ vcol, const unsigned char* __restrict__ fcol,
                        unsigned char* __restrict__ out_u8, int S, int row0, int col0, int ph, int pw, int low_x, int br, int bg, int bb)
{
    const int b = blockIdx.y;
    const int px = blockIdx.x * kBlock + threadIdx.x;
    if (px >= ph * pw) return;
    const size_t o = (size_t)b * ph * pw + px;
    const i64 t = tri_id[o];
    i64 v0, v1, t0, t1;
    mesh_slice(ms, mesh_of_item[b], v0, v1, t0, t1);
    int rgb[3] = {br, bg, bb};
    if (t >= 0 && t < t1 - t0 && v1 > v0) {
        if (fcol) {
#pragma unroll
            for (int j = 0; j < 3; ++j) rgb[j] = fcol[3 * (t0 + t) + j];
        } else {
            int p[3][3];
            i64 vid[3];
            ScreenTri s;
            s.A = 0;                                             // stays 0 when the setup stops at a zero lattice normal or a zero area
            load_tri(ms, v0, v1, t0 + t, S, p, vid);
            // the resolve's setup, culling off; an empty pixel box (an id the rasteriser did not write) still leaves s wound
            screen_setup(p, cam + (size_t)b * 12, 0, low_x, row0, col0, ph, pw, s);
            if (s.A <= 0) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    rgb[j] = (2 * ((int)vcol[3 * vid[0] + j] + (int)vcol[3 * vid[1] + j] + (int)vcol[3 * vid[2] + j]) + 3) / 6;
            } else {
                i64 E[3];
                edge_functions(s, row0 + px / pw, col0 + px % pw, E);
                // vertex at wound position k carries E_(k+1): as Z in the depth and the normals in the resolve
                const i64 w[3] = {E[1], E[2], E[0]};
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    i64 n = 0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) n += w[k] * (i64)vcol[3 * vid[s.order[k]] + j];
                    rgb[j] = (int)clampi(floor_div(2 * n + s.A, 2 * s.A), 0, 255);      // |2 n + A| < 2^54
                }
            }
        }
    }
    out_u8[o * 3 + 0] = (unsigned char)rgb[0];
    out_u8[o * 3 + 1] = (unsigned char)rgb[1];
    out_u8[o * 3 + 2] = (unsigned char)rgb[2];
}

// ---- the voxel behind a face of a surface net -----------------------------------------------------------------------------------

// thread = face; its grid is the last b with face_offsets[b] <= f, searched inside 0 .. B-1 whatever the offsets hold
template <typename T>
__global__ __launch_bounds__(kBlock)
void mesh_face_voxels_kernel(const int* __restrict__ verts, i64 V, const i64* __restrict__ vert_offsets, const int* __restrict__ faces,
                             i64 F, int width, const i64* __restrict__ face_offsets, const T* __restrict__ vol, float threshold,
                             int* __restrict__ out, int B, int S)
{
    const i64 f = (i64)blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (face_offsets[mid] <= f) lo = mid; else hi = mid - 1;
    }
    const i64 v0 = clampi(vert_offsets[lo], 0, V), v1 = clampi(vert_offsets[lo + 1], v0, V);
    const i64 f0 = clampi(face_offsets[lo], 0, F), f1 = clampi(face_offsets[lo + 1], f0, F);
    int id = -1;
    if (f >= f0 && f < f1 && v1 > v0) {
        i64 c[3][3];                                             // c[k][j]: cell of the face's vertex k, array axis j
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const i64 v = v0 + clampi((i64)faces[f * width + k], 0, v1 - v0 - 1);
#pragma unroll
            for (int j = 0; j < 3; ++j) c[k][j] = (((i64)verts[3 * v + j] + 128) >> 8) - 1;
        }
        int a = 0, shared = 0;
        bool ring = true;                                        // vertices 1 and 2 lie in c .. c + 1 on every axis
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const i64 d1 = c[1][j] - c[0][j], d2 = c[2][j] - c[0][j];
            ring = ring && (d1 == 0 || d1 == 1) && (d2 == 0 || d2 == 1);
            if (d1 == 0 && d2 == 0) { a = j; ++shared; }
        }
        if (ring && shared == 1) {
            const int u = (a + 1) % 3, w = (a + 2) % 3;
            i64 s[3];
            s[a] = c[0][a];
            s[u] = c[0][u] + 1;
            s[w] = c[0][w] + 1;
            if (s[u] >= 0 && s[u] < S && s[w] >= 0 && s[w] < S) {
                const T* g = vol + (size_t)lo * S * S * S;
                bool in[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {                    // the edge's two ends; a sample outside the grid is outside
                    i64 x[3] = {s[0], s[1], s[2]};
                    x[a] += e;
                    in[e] = x[a] >= 0 && x[a] < S && (float)g[((size_t)x[0] * S + x[1]) * S + x[2]] > threshold;
                }
                if (in[0] != in[1]) {
                    s[a] += in[1] ? 1 : 0;
                    id = (int)((s[0] * S + s[1]) * S + s[2]);
                }
            }
        }
    }
    out[f] = id;
}

int check_set(const char* what, const int* verts, long long V, const int* tris, long long T, const long long* vo,
              const long long* to, int M, int S)
{
    if (rn_check_grid_side_pow2(what, S)) return RN_E_INVALID;
    if (V < 0 || T < 0 || V > (1ll << 28) || T > (1ll << 28) || (T > 0 && V == 0))
        return rn_set_error(RN_E_INVALID, "%s: V=%lld T=%lld (at most 2^28 each, no triangles without vertices)", what, V, T);
    if (M < 1 || M > 65535) return rn_set_error(RN_E_INVALID, "%s: %d meshes (1..65535)", what, M);
    return rn_check_pointers(what, {vo, to}) || (V > 0 && rn_check_pointers(what, {verts})) || (T > 0 && rn_check_pointers(what, {tris})) ||
           rn_check_aligned(what, vo, 8, "vert_offsets") || rn_check_aligned(what, to, 8, "tri_offsets") ||
           rn_check_aligned(what, verts, 4, "verts") || rn_check_aligned(what, tris, 4, "tris");
}

int check_camera(const char* what, int B, int N, int f)
{
    if (rn_check_batch(what, B)) return RN_E_INVALID;
    if (N < 1 || N > 256 || f < 1 || f > 16 || f * N > 2048)
        return rn_set_error(RN_E_INVALID, "%s: N=%d, pixels_per_cell=%d (N <= 256, f <= 16, f N <= 2048)", what, N, f);
    return RN_OK;
}

}  // namespace

extern "C" int rn_mesh_camera(const float* m_inv, long long* cam, int B, int N, int pixels_per_cell, int view_from_low_x, void* stream)
{
    if (check_camera(__func__, B, N, pixels_per_cell)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(__func__, {m_inv, cam}) || rn_check_aligned(__func__, m_inv, 4, "m_inv") || rn_check_aligned(__func__, cam, 8, "cam"))
        return RN_E_INVALID;
    hipLaunchKernelGGL(mesh_camera_kernel, dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       m_inv, cam, B, N, pixels_per_cell, view_from_low_x ? 1 : 0, (u64*)nullptr, (size_t)0);
    return rn_check_launch(__func__);
}

extern "C" int rn_mesh_vertex_normals(const int* verts, long long V, const int* tris, long long T, const long long* vert_offsets,
                                      const long long* tri_offsets, int M, int S, long long* vnorm, void* stream)
{
    if (check_set(__func__, verts, V, tris, T, vert_offsets, tri_offsets, M, S)) return RN_E_INVALID;
    if (V == 0) return RN_OK;
    if (rn_check_pointers(__func__, {vnorm}) || rn_check_aligned(__func__, vnorm, 8, "vnorm")) return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)V * 3;
    hipLaunchKernelGGL(mesh_clear_i64_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, vnorm, n);
    if (T > 0) {
        const Meshes ms = {verts, V, tris, T, vert_offsets, tri_offsets, M};
        hipLaunchKernelGGL(mesh_vnormal_kernel, dim3((unsigned)((T + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, ms, S, vnorm);
    }
    return rn_check_launch(__func__);
}

extern "C" int rn_mesh_rasterize(const int* verts, long long V, const int* tris, long long T, const long long* vert_offsets,
                                 const long long* tri_offsets, int M, const int* mesh_of_item, long long max_tris,
                                 const float* m_inv, const long long* vnorm, long long* cam, unsigned long long* keys,
                                 unsigned char* out_u8, int* tri_id, int* depth, int B, int S, int N, int pixels_per_cell,
                                 int row0, int col0, int ph, int pw, int cull, int view_from_low_x, void* stream)
{
    const char* what = __func__;
    if (check_set(what, verts, V, tris, T, vert_offsets, tri_offsets, M, S) || check_camera(what, B, N, pixels_per_cell)) return RN_E_INVALID;
    const int side = pixels_per_cell * N;
    if (ph < 1 || pw < 1 || row0 < 0 || col0 < 0 || row0 > side - ph || col0 > side - pw)
        return rn_set_error(RN_E_INVALID, "%s: window (%d, %d, %d, %d) outside the %d x %d frame", what, row0, col0, ph, pw, side, side);
    if (cull != RN_CULL_NONE && cull != RN_CULL_BACK) return rn_set_error(RN_E_INVALID, "%s: cull=%d (0 none, 1 back)", what, cull);
    if (max_tris < 0 || max_tris > T) return rn_set_error(RN_E_INVALID, "%s: max_tris=%lld for T=%lld", what, max_tris, T);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {mesh_of_item, m_inv, cam, keys, out_u8}) || rn_check_aligned(what, mesh_of_item, 4, "mesh_of_item") ||
        rn_check_aligned(what, m_inv, 4, "m_inv") || rn_check_aligned(what, tri_id, 4, "tri_id") ||
        rn_check_aligned(what, depth, 4, "depth") || rn_check_aligned(what, cam, 8, "cam") || rn_check_aligned(what, keys, 8, "keys") ||
        rn_check_aligned(what, vnorm, 8, "vnorm"))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t n_keys = (size_t)B * ph * pw;                   // <= 65535 * 2^22
    const Meshes ms = {verts, V, tris, T, vert_offsets, tri_offsets, M};
    const int low_x = view_from_low_x ? 1 : 0;
    const unsigned clear_blocks = (unsigned)min((n_keys + kBlock - 1) / kBlock, (size_t)8192);   // >= ceil(B / 256): B <= 65535 < n_keys
    hipLaunchKernelGGL(mesh_camera_kernel, dim3(max(clear_blocks, (unsigned)((B + kBlock - 1) / kBlock))), dim3(kBlock), 0, st,
                       m_inv, cam, B, N, pixels_per_cell, low_x, keys, n_keys);
    if (max_tris > 0)
        hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)((max_tris + kBlock - 1) / kBlock), (unsigned)B), dim3(kBlock), 0, st,
                           ms, mesh_of_item, (const i64*)cam, keys, S, N, row0, col0, ph, pw, cull == RN_CULL_BACK ? 1 : 0, low_x);
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((ph * pw + kBlock - 1) / kBlock), (unsigned)B), dim3(kBlock), 0, st,
                       ms, mesh_of_item, (const i64*)cam, m_inv, (const i64*)vnorm, (const u64*)keys, out_u8, tri_id, depth,
                       S, row0, col0, ph, pw, low_x);
    return rn_check_launch(what);
}

extern "C" int rn_mesh_colour_from_ids(const int* verts, long long V, const int* tris, long long T, const long long* vert_offsets,
                                       const long long* tri_offsets, int M, const int* mesh_of_item, const long long* cam,
                                       const int* tri_id, const unsigned char* vcol, const unsigned char* fcol,
                                       unsigned char* out_u8, int B, int S, int N, int pixels_per_cell, int row0, int col0, int ph,
                                       int pw, int view_from_low_x, int background_r, int background_g, int background_b, void* stream)
{
    const char* what = __func__;
    if (check_set(what, verts, V, tris, T, vert_offsets, tri_offsets, M, S) ||
        rn_check_frame(what, B, N, pixels_per_cell, row0, col0, ph, pw))
        return RN_E_INVALID;
    if ((vcol == nullptr) == (fcol == nullptr))
        return rn_set_error(RN_E_INVALID, "%s: exactly one of vcol and fcol", what);
    if (background_r < 0 || background_r > 255 || background_g < 0 || background_g > 255 || background_b < 0 || background_b > 255)
        return rn_set_error(RN_E_INVALID, "%s: background (%d, %d, %d), each 0..255", what, background_r, background_g, background_b);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {mesh_of_item, cam, tri_id, out_u8}) || rn_check_aligned(what, mesh_of_item, 4, "mesh_of_item") ||
        rn_check_aligned(what, tri_id, 4, "tri_id") || rn_check_aligned(what, cam, 8, "cam"))
        return RN_E_INVALID;
    const Meshes ms = {verts, V, tris, T, vert_offsets, tri_offsets, M};
    hipLaunchKernelGGL(mesh_colour_kernel, dim3((unsigned)((ph * pw + kBlock - 1) / kBlock), (unsigned)B), dim3(kBlock), 0,
                       (hipStream_t)stream, ms, mesh_of_item, (const i64*)cam, tri_id, vcol, fcol, out_u8, S, row0, col0, ph, pw,
                       view_from_low_x ? 1 : 0, background_r, background_g, background_b);
    return rn_check_launch(what);
}

extern "C" int rn_mesh_face_voxels(const int* verts, long long V, const long long* vert_offsets, const int* faces, long long F,
                                   int width, const long long* face_offsets, const void* vol, int vol_is_u8, float threshold,
                                   int* out, int B, int S, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || rn_check_grid_side_pow2(what, S)) return RN_E_INVALID;
    if (V < 0 || F < 0 || V > (1ll << 28) || F > (1ll << 28))
        return rn_set_error(RN_E_INVALID, "%s: V=%lld F=%lld (at most 2^28 each)", what, V, F);
    if (width != 3 && width != 4) return rn_set_error(RN_E_INVALID, "%s: width=%d (3 triangles, 4 quads)", what, width);
    if (vol_is_u8 != 0 && vol_is_u8 != 1) return rn_set_error(RN_E_INVALID, "%s: vol_is_u8=%d", what, vol_is_u8);
    if (!(threshold == threshold)) return rn_set_error(RN_E_INVALID, "%s: threshold is NaN", what);
    if (B == 0 && F != 0) return rn_set_error(RN_E_INVALID, "%s: %lld faces of no grid", what, F);
    if (B == 0 || F == 0) return RN_OK;
    if (rn_check_pointers(what, {vert_offsets, faces, face_offsets, vol, out}) || (V > 0 && rn_check_pointers(what, {verts})) ||
        rn_check_aligned(what, verts, 4, "verts") || rn_check_aligned(what, faces, 4, "faces") || rn_check_aligned(what, out, 4, "out") ||
        rn_check_aligned(what, vert_offsets, 8, "vert_offsets") || rn_check_aligned(what, face_offsets, 8, "face_offsets") ||
        rn_check_aligned(what, vol, vol_is_u8 ? 1 : 4, "vol"))
        return RN_E_INVALID;
    const dim3 grid((unsigned)((F + kBlock - 1) / kBlock));
    if (vol_is_u8)
        hipLaunchKernelGGL(mesh_face_voxels_kernel<unsigned char>, grid, dim3(kBlock), 0, (hipStream_t)stream, verts, (i64)V,
                           (const i64*)vert_offsets, faces, (i64)F, width, (const i64*)face_offsets, (const unsigned char*)vol, threshold,
                           out, B, S);
    else
        hipLaunchKernelGGL(mesh_face_voxels_kernel<float>, grid, dim3(kBlock), 0, (hipStream_t)stream, verts, (i64)V,
                           (const i64*)vert_offsets, faces, (i64)F, width, (const i64*)face_offsets, (const float*)vol, threshold, out,
                           B, S);
    return rn_check_launch(what);
}
