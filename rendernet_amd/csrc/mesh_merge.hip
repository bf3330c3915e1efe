// Merged blocky mesh: the exposed voxel faces of a grid merged into rectangles, run by run (gfx950).  The rule -- inside set,
// labels, planes, runs, rectangles, quads, vertices and their order -- is stated once in include/rendernet_hip.h
// (rn_mesh_merge_count / rn_mesh_merge_emit); the NumPy twin is tests/mesh_merge_ref.py.  Integer arithmetic apart from the
// comparison with the threshold.
//
// Everything after the first kernel works on ROW WORDS: bit v of the word of (axis a, slice s, row u) = the sample with s on a,
// u on u and v on v is inside; one 64-bit word up to 64^3, one 128-bit word at 128^3.  With labels a second word holds, per
// sample, "my label differs from the one at v - 1".  The face mask of plane k and a side is then lo & ~hi of two slice words,
// the run starts and ends are shifts of it, and "row u - 1 holds the identical run" is three masked comparisons and, with
// labels, one label read.  No atomic decides an index: the quads are numbered by the stream compaction of voxel_common.h over
// the threads in (a, k, side, u) order, each thread emitting its row's rectangles by rising v0; the vertices by the same
// compaction over the (S + 1)^3 corner marks, which are plain stores of 1.
//
//   merge_pack_kernel      one thread per (a, slice, row) walks v: the row word and the label-change word.  Threads run along
//                          array axis 2 wherever that is not the walk's own axis, so that a wave reads whole lines
//   merge_count_kernel     one thread per (a, k, side, u): the runs of its row that start a rectangle, their heights by walking
//                          the rows below, the four corner marks; the workgroup's rectangles go to the workspace
//   merge_marks_kernel     the marked corners of each workgroup of 256 corners
//   merge_scan_kernel      one workgroup per grid: exclusive prefixes of both lists of totals in place, the grid's (V, F)
//   merge_verts_kernel     vertex id = the rank of the corner among the marked ones; writes q and the corner -> id volume
//   merge_quads_kernel     the rows again; quad index = the workgroup's prefix + the rank of the row's first rectangle
#include "voxel_common.h"
#include "rn_checks.h"

namespace {

constexpr int kAhead = 8;                                        // samples of a row that merge_pack_kernel loads before it tests any

typedef unsigned long long Word64;
typedef unsigned __int128 Word128;

__device__ __forceinline__ int low_bit(Word64 w) { return __builtin_ctzll(w); }                  // w != 0
__device__ __forceinline__ int low_bit(Word128 w)
{
    const Word64 lo = (Word64)w;
    return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((Word64)(w >> 64));
}

struct Layout {                                                  // byte offsets into the workspace, each a multiple of 16
    size_t bits, diff, marks, ids, qtot, vtot, total;
    int nbq, nbv;
};

size_t up16(size_t n) { return (n + 15) / 16 * 16; }

Layout layout_of(int B, int S)
{
    Layout l;
    const size_t N = (size_t)S + 1, rows = (size_t)B * 3 * S * S, word = S == 128 ? 16 : 8;
    l.nbq = (3 * (S + 1) * 2 * S + kBlock - 1) / kBlock;
    l.nbv = (int)((N * N * N + kBlock - 1) / kBlock);
    l.bits = 0;
    l.diff = l.bits + up16(rows * word);
    l.marks = l.diff + up16(rows * word);
    l.ids = l.marks + up16((size_t)B * N * N * N);
    l.qtot = l.ids + up16((size_t)B * N * N * N * 4);
    l.vtot = l.qtot + up16((size_t)B * l.nbq * 4);
    l.total = l.vtot + up16((size_t)B * l.nbv * 4);
    return l;
}

template <typename T, typename Word>
__global__ __launch_bounds__(kBlock)
void merge_pack_kernel(const T* __restrict__ vol, const int* __restrict__ labels, float threshold, int S, Word* __restrict__ bits,
                       Word* __restrict__ diff)
{
    const int t = blockIdx.x * kBlock + threadIdx.x, b = blockIdx.y;
    if (t >= 3 * S * S) return;
    const int a = t / (S * S), r = t - a * S * S, x = r / S, y = r - x * S;
    const int slice = a == 2 ? y : x, row = a == 2 ? x : y;      // the fastest thread index runs along array axis 2 for a = 1, 2
    const int u = a == 2 ? 0 : a + 1, v = u == 2 ? 0 : u + 1;
    const int stride[3] = {S * S, S, 1};
    const size_t base = (size_t)b * S * S * S + (size_t)slice * stride[a] + (size_t)row * stride[u];
    Word m = 0, d = 0;
    int before = 0;
    for (int i0 = 0; i0 < S; i0 += kAhead) {                     // S is a multiple of kAhead: the loads of a chunk are in flight together
        float value[kAhead];
        int label[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const size_t at = base + (size_t)(i0 + j) * stride[v];
            value[j] = (float)vol[at];
            label[j] = labels ? labels[at] : 0;
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            if (value[j] > threshold) m |= (Word)1 << (i0 + j);
            if (i0 + j == 0 || label[j] != before) d |= (Word)1 << (i0 + j);
            before = label[j];
        }
    }
    const size_t out = (((size_t)b * 3 + a) * S + slice) * S + row;
    bits[out] = m;
    if (labels) diff[out] = d;
}

// one (grid, axis, plane, side): what a thread of the count and the quads kernels reads its rows through
template <typename Word>
struct Plane {
    const Word* bits;                                            // of the grid and the axis: [S slices][S rows]
    const Word* diff;
    const int* labels;                                           // of the grid, or null
    int S, a, k, side, inside;                                   // inside: the slice of the inside voxels, k - 1 or k
};

template <typename Word>
struct Row { Word mask, first, last; };                          // the faces of a row, those that start a run, those that end one

template <typename Word>
__device__ __forceinline__ Row<Word> row_of(const Plane<Word>& p, int u)
{
    const Word lo = p.k > 0 ? p.bits[(p.k - 1) * p.S + u] : (Word)0, hi = p.k < p.S ? p.bits[p.k * p.S + u] : (Word)0;
    const Word m = p.side ? hi & ~lo : lo & ~hi;
    const Word d = p.labels ? p.diff[p.inside * p.S + u] : (Word)0;
    return {m, m & (~(m << 1) | d), m & (~(m >> 1) | (d >> 1))};
}

template <typename Word>
__device__ __forceinline__ int label_at(const Plane<Word>& p, int u, int v)
{
    const int ua = p.a == 2 ? 0 : p.a + 1, va = ua == 2 ? 0 : ua + 1;
    int s[3];
    s[p.a] = p.inside;
    s[ua] = u;
    s[va] = v;
    return p.labels[((size_t)s[0] * p.S + s[1]) * p.S + s[2]];
}

// the row holds exactly the run `run` = bits v0 .. v1 - 1: all faces, one start, one end
template <typename Word>
__device__ __forceinline__ bool holds_run(const Row<Word>& r, Word run, int v0, int v1)
{
    return (r.mask & run) == run && (r.first & run) == (Word)1 << v0 && (r.last & run) == (Word)1 << (v1 - 1);
}

// f(v0, v1, height) for every run of row u that starts a rectangle, by rising v0; height is 1 unless `heights`
template <typename Word, typename F>
__device__ __forceinline__ void for_each_rectangle(const Plane<Word>& p, int u, bool heights, F&& f)
{
    constexpr int kBits = 8 * sizeof(Word);
    const Row<Word> row = row_of(p, u);
    if (!row.first) return;
    Row<Word> above = {0, 0, 0};
    if (u > 0) above = row_of(p, u - 1);
    for (Word left = row.first; left; left &= left - 1) {
        const int v0 = low_bit(left);
        const Word ends = row.last >> v0;
        const int v1 = v0 + (ends ? low_bit(ends) : 0) + 1;      // a run always ends: `ends` is never 0
        const Word run = (~(Word)0 >> (kBits - (v1 - v0))) << v0;
        const int key = p.labels ? label_at(p, u, v0) : 0;
        if (u > 0 && holds_run(above, run, v0, v1) && (!p.labels || label_at(p, u - 1, v0) == key)) continue;
        int h = 1;
        if (heights)
            for (int w = u + 1; w < p.S; ++w, ++h)
                if (!holds_run(row_of(p, w), run, v0, v1) || (p.labels && label_at(p, w, v0) != key)) break;
        f(v0, v1, h);
    }
}

// the plane and the row of a thread of the count and the quads kernels; false past the last row
template <typename Word>
__device__ __forceinline__ bool plane_of_thread(int i, int b, int S, const Word* bits, const Word* diff, const int* labels,
                                                Plane<Word>* p, int* u)
{
    if (i >= 3 * (S + 1) * 2 * S) return false;
    const int plane = i / (2 * S), r = i - plane * 2 * S;
    p->S = S;
    p->a = plane / (S + 1);
    p->k = plane - p->a * (S + 1);
    p->side = r / S;
    p->inside = min(max(p->k - 1 + p->side, 0), S - 1);          // a border plane's missing side has no faces
    p->bits = bits + ((size_t)b * 3 + p->a) * S * S;
    p->diff = diff + ((size_t)b * 3 + p->a) * S * S;
    p->labels = labels ? labels + (size_t)b * S * S * S : nullptr;
    *u = r - p->side * S;
    return true;
}

// the flat index of the lattice corner with k on a, cu on u and cv on v
__device__ __forceinline__ int corner_of(int N, int a, int k, int cu, int cv)
{
    const int ua = a == 2 ? 0 : a + 1, va = ua == 2 ? 0 : ua + 1;
    int c[3];
    c[a] = k;
    c[ua] = cu;
    c[va] = cv;
    return (c[0] * N + c[1]) * N + c[2];
}

template <typename Word>
__global__ __launch_bounds__(kBlock)
void merge_count_kernel(const Word* __restrict__ bits, const Word* __restrict__ diff, const int* __restrict__ labels, int S, int nb,
                        unsigned char* __restrict__ marks, int* __restrict__ qtot)
{
    __shared__ int red[kWaves];
    const int N = S + 1, b = blockIdx.y;
    Plane<Word> p;
    int u, n = 0;
    if (plane_of_thread(blockIdx.x * kBlock + threadIdx.x, b, S, bits, diff, labels, &p, &u)) {
        unsigned char* mine = marks + (size_t)b * N * N * N;
        for_each_rectangle(p, u, true, [&](int v0, int v1, int h) {
            ++n;
            mine[corner_of(N, p.a, p.k, u, v0)] = 1;
            mine[corner_of(N, p.a, p.k, u + h, v0)] = 1;
            mine[corner_of(N, p.a, p.k, u + h, v1)] = 1;
            mine[corner_of(N, p.a, p.k, u, v1)] = 1;
        });
    }
    const int total = block_sum(n, red);
    if (threadIdx.x == 0) qtot[(size_t)b * nb + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock)
void merge_marks_kernel(const unsigned char* __restrict__ marks, int S, int nb, int* __restrict__ vtot)
{
    __shared__ int sv[kWaves];
    const int N = S + 1, corners = N * N * N, b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool used = i < corners && marks[(size_t)b * corners + i] != 0;
    const int n = block_count((int)__popcll(__ballot(used)), sv);
    if (threadIdx.x == 0) vtot[(size_t)b * nb + blockIdx.x] = n;
}

__global__ __launch_bounds__(kBlock)
void merge_scan_kernel(int* __restrict__ vtot, int nbv, int* __restrict__ qtot, int nbq, int* __restrict__ totals)
{
    __shared__ int swave[kWaves];
    const int verts = scan_totals(vtot + (size_t)blockIdx.x * nbv, nbv, swave);
    const int quads = scan_totals(qtot + (size_t)blockIdx.x * nbq, nbq, swave);
    if (threadIdx.x == 0) {
        totals[2 * blockIdx.x] = verts;
        totals[2 * blockIdx.x + 1] = quads;
    }
}

__global__ __launch_bounds__(kBlock)
void merge_verts_kernel(const unsigned char* __restrict__ marks, int S, int nb, const int* __restrict__ vtot,
                        const long long* __restrict__ vert_offsets, long long n_verts, int* __restrict__ ids, int* __restrict__ q)
{
    __shared__ int sv[kWaves];
    const int N = S + 1, corners = N * N * N, b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool used = i < corners && marks[(size_t)b * corners + i] != 0;
    const unsigned long long vote = __ballot(used);
    const int id = vtot[(size_t)b * nb + blockIdx.x] + block_rank(__popcll(vote), lanes_before(vote), sv);
    if (i >= corners) return;
    ids[(size_t)b * corners + i] = used ? id : -1;
    if (!used) return;
    const long long at = vert_offsets[b] + id;
    if (at < 0 || at >= n_verts) return;                         // offsets that do not belong to this workspace write nothing
    q[3 * at] = 256 * (i / (N * N));
    q[3 * at + 1] = 256 * (i / N % N);
    q[3 * at + 2] = 256 * (i % N);
}

template <typename Word, bool kTriangles>
__global__ __launch_bounds__(kBlock)
void merge_quads_kernel(const Word* __restrict__ bits, const Word* __restrict__ diff, const int* __restrict__ labels, int S, int nb,
                        const int* __restrict__ qtot, const int* __restrict__ ids, const long long* __restrict__ quad_offsets,
                        long long n_quads, int* __restrict__ faces, int* __restrict__ face_voxel, int* __restrict__ face_dir,
                        int* __restrict__ face_size)
{
    __shared__ int sq[kWaves];
    const int N = S + 1, b = blockIdx.y, lane = threadIdx.x & (kWave - 1);
    Plane<Word> p;
    int u, n = 0;
    const bool live = plane_of_thread(blockIdx.x * kBlock + threadIdx.x, b, S, bits, diff, labels, &p, &u);
    if (live) for_each_rectangle(p, u, false, [&](int, int, int) { ++n; });
    int upto = n;                                                // the inclusive scan of n down the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl_up(upto, d);
        if (lane >= d) upto += t;
    }
    int k = qtot[(size_t)b * nb + blockIdx.x] + block_rank(__shfl(upto, kWave - 1), upto - n, sq);
    if (n == 0) return;
    const int* id = ids + (size_t)b * N * N * N;
    const int ua = p.a == 2 ? 0 : p.a + 1, va = ua == 2 ? 0 : ua + 1;
    for_each_rectangle(p, u, true, [&](int v0, int v1, int h) {
        const long long at = quad_offsets[b] + k;
        ++k;
        if (at < 0 || at >= n_quads) return;                     // never for the offsets of this workspace
        const int r0 = id[corner_of(N, p.a, p.k, u, v0)], r1 = id[corner_of(N, p.a, p.k, u + h, v0)],
                  r2 = id[corner_of(N, p.a, p.k, u + h, v1)], r3 = id[corner_of(N, p.a, p.k, u, v1)];
        const int s1 = p.side ? r3 : r1, s3 = p.side ? r1 : r3;  // side 1: the ring (0, 3, 2, 1), the normal is -a
        if (kTriangles) {
            int2* out = (int2*)(faces + 6 * at);                 // (0,1,2), (0,2,3)
            out[0] = make_int2(r0, s1);
            out[1] = make_int2(r2, r0);
            out[2] = make_int2(r2, s3);
        } else {
            ((int4*)faces)[at] = make_int4(r0, s1, r2, s3);
        }
        int s[3];
        s[p.a] = p.inside;
        s[ua] = u;
        s[va] = v0;
        face_voxel[at] = (s[0] * S + s[1]) * S + s[2];
        face_dir[at] = 2 * p.a + p.side;
        ((int2*)face_size)[at] = make_int2(h, v1 - v0);
    });
}

// the checks the two entries share; 0 when the arguments are fine
int check_common(const char* who, int B, int S, const int* labels, const void* ws, size_t ws_bytes)
{
    if (rn_check_grid_side_pow2(who, S) || rn_check_batch(who, B)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    return rn_check_aligned(who, labels, 4, "labels") || rn_check_ws(who, ws, ws_bytes, rn_mesh_merge_workspace_bytes(B, S));
}

template <typename T, typename Word>
void launch_count(const void* vol, const int* labels, float threshold, int B, int S, char* ws, const Layout& l, int* totals,
                  hipStream_t st)
{
    Word* bits = (Word*)(ws + l.bits);
    Word* diff = (Word*)(ws + l.diff);
    unsigned char* marks = (unsigned char*)(ws + l.marks);
    int* qtot = (int*)(ws + l.qtot);
    int* vtot = (int*)(ws + l.vtot);
    const dim3 block(kBlock);
    hipLaunchKernelGGL((merge_pack_kernel<T, Word>), dim3((unsigned)((3 * S * S + kBlock - 1) / kBlock), (unsigned)B), block, 0, st,
                       (const T*)vol, labels, threshold, S, bits, diff);
    hipLaunchKernelGGL((merge_count_kernel<Word>), dim3((unsigned)l.nbq, (unsigned)B), block, 0, st, (const Word*)bits,
                       (const Word*)diff, labels, S, l.nbq, marks, qtot);
    hipLaunchKernelGGL(merge_marks_kernel, dim3((unsigned)l.nbv, (unsigned)B), block, 0, st, (const unsigned char*)marks, S, l.nbv, vtot);
    hipLaunchKernelGGL(merge_scan_kernel, dim3((unsigned)B), block, 0, st, vtot, l.nbv, qtot, l.nbq, totals);
}

template <typename Word>
void launch_quads(const int* labels, int B, int S, int triangles, const char* ws, const Layout& l, const long long* quad_offsets,
                  long long n_quads, int* faces, int* face_voxel, int* face_dir, int* face_size, hipStream_t st)
{
    const Word* bits = (const Word*)(ws + l.bits);
    const Word* diff = (const Word*)(ws + l.diff);
    const int* qtot = (const int*)(ws + l.qtot);
    const int* ids = (const int*)(ws + l.ids);
    const dim3 grid((unsigned)l.nbq, (unsigned)B), block(kBlock);
    if (triangles)
        hipLaunchKernelGGL((merge_quads_kernel<Word, true>), grid, block, 0, st, bits, diff, labels, S, l.nbq, qtot, ids, quad_offsets,
                           n_quads, faces, face_voxel, face_dir, face_size);
    else
        hipLaunchKernelGGL((merge_quads_kernel<Word, false>), grid, block, 0, st, bits, diff, labels, S, l.nbq, qtot, ids, quad_offsets,
                           n_quads, faces, face_voxel, face_dir, face_size);
}

}  // namespace

extern "C" size_t rn_mesh_merge_workspace_bytes(int B, int S)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B)) return 0;
    return layout_of(B, S).total;
}

extern "C" int rn_mesh_merge_count(const void* vol, int vol_is_u8, const int* labels, float threshold, int B, int S, void* workspace,
                                   size_t workspace_bytes, int* totals, void* stream)
{
    const char* who = __func__;
    if (rn_check_grid_side_pow2(who, S) || rn_check_batch(who, B)) return RN_E_INVALID;
    if (vol_is_u8 != 0 && vol_is_u8 != 1) return rn_set_error(RN_E_INVALID, "%s: vol_is_u8=%d", who, vol_is_u8);
    if (!(threshold == threshold)) return rn_set_error(RN_E_INVALID, "%s: threshold is NaN", who);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(who, {vol, totals}) || rn_check_aligned(who, vol, vol_is_u8 ? 1 : 4, "vol") ||
        rn_check_aligned(who, totals, 4, "totals") || check_common(who, B, S, labels, workspace, workspace_bytes))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout_of(B, S);
    char* ws = (char*)workspace;
    const size_t N = (size_t)S + 1;
    if (hipMemsetAsync(ws + l.marks, 0, (size_t)B * N * N * N, st) != hipSuccess)
        return rn_set_error(RN_E_INVALID, "%s: clearing the corner marks failed", who);
    if (S == 128) {
        if (vol_is_u8) launch_count<unsigned char, Word128>(vol, labels, threshold, B, S, ws, l, totals, st);
        else launch_count<float, Word128>(vol, labels, threshold, B, S, ws, l, totals, st);
    } else {
        if (vol_is_u8) launch_count<unsigned char, Word64>(vol, labels, threshold, B, S, ws, l, totals, st);
        else launch_count<float, Word64>(vol, labels, threshold, B, S, ws, l, totals, st);
    }
    return rn_check_launch(who);
}

extern "C" int rn_mesh_merge_emit(const int* labels, int B, int S, int triangles, void* workspace, size_t workspace_bytes,
                                  const long long* vert_offsets, const long long* quad_offsets, long long n_verts, long long n_quads,
                                  int* q, int* faces, int* face_voxel, int* face_dir, int* face_size, void* stream)
{
    const char* who = __func__;
    if (check_common(who, B, S, labels, workspace, workspace_bytes)) return RN_E_INVALID;
    if (triangles != 0 && triangles != 1) return rn_set_error(RN_E_INVALID, "%s: triangles=%d", who, triangles);
    if (n_verts < 0 || n_quads < 0) return rn_set_error(RN_E_INVALID, "%s: n_verts=%lld n_quads=%lld", who, n_verts, n_quads);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(who, {vert_offsets, quad_offsets}) || (n_verts > 0 && rn_check_pointers(who, {q})) ||
        (n_quads > 0 && rn_check_pointers(who, {faces, face_voxel, face_dir, face_size})) ||
        rn_check_aligned(who, vert_offsets, 8, "vert_offsets") || rn_check_aligned(who, quad_offsets, 8, "quad_offsets") ||
        rn_check_aligned(who, q, 4, "q") || rn_check_aligned(who, faces, 16, "faces") ||
        rn_check_aligned(who, face_voxel, 4, "face_voxel") || rn_check_aligned(who, face_dir, 4, "face_dir") ||
        rn_check_aligned(who, face_size, 8, "face_size"))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout_of(B, S);
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(merge_verts_kernel, dim3((unsigned)l.nbv, (unsigned)B), dim3(kBlock), 0, st,
                       (const unsigned char*)(ws + l.marks), S, l.nbv, (const int*)(ws + l.vtot), vert_offsets, n_verts,
                       (int*)(ws + l.ids), q);
    if (n_quads > 0) {
        if (S == 128) launch_quads<Word128>(labels, B, S, triangles, ws, l, quad_offsets, n_quads, faces, face_voxel, face_dir, face_size, st);
        else launch_quads<Word64>(labels, B, S, triangles, ws, l, quad_offsets, n_quads, faces, face_voxel, face_dir, face_size, st);
    }
    return rn_check_launch(who);
}
