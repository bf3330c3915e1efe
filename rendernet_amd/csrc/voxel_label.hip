// Exact connected-component labelling of packed occupancy grids, the per-component statistics and the topology words built on
// it (gfx950).  Integer arithmetic throughout, no float, no inline assembly; the rule is stated in include/rendernet_hip.h
// (rn_voxel_label / rn_voxel_label_stats / rn_voxel_topology), the NumPy twin is tests/voxel_label_ref.py.
//
// One thread per voxel, 256-thread workgroups, lanes along xs, grid (S^3 / 256, B).  The union-find array is the `labels` output
// itself (parent = flat index inside the item, -1 on an unselected voxel; the invariant is parent[i] <= i, and parents only
// decrease, so a component's root ends as its minimum flat index whatever order the atomics arrive in):
//   label_init_kernel     parent = the start of the voxel's run along xs, from clz on the masked row words: x-adjacency costs no
//                         union.  Clears the voxel's word of the flag / rank array.
//   label_merge_kernel    every selected voxel x looks at the earlier neighbour rows (2 for 6-connectivity, 4 with dx = -1, 0, 1
//                         for 26).  The pair (x, p) is united unless (x, p - 1) or (x - 1, p - 1) is a pair too: either joins
//                         the same two runs, and every chain of such steps ends at a pair that is united.  Decided per raw run:
//                         a voxel between two runs of a neighbour row unites with both.  Union: find both roots, atomicMin the
//                         larger root's parent with the smaller, go on with the value returned until the roots agree.  In this launch every read of the array
//                         is a relaxed agent-scope atomic load and every write an agent-scope atomicMin (a find also lowers its
//                         starting voxel's parent to the root it reached: an ancestor, so the invariant and the sets stand).
//   label_flatten_kernel  every voxel chases to its root with plain loads (nothing writes the array in this launch) and writes it
//                         to a second array; for the empty space a border voxel ORs the outside flag into its root's flag word.
//   label_count / _scan / _emit   flag the roots that are not outside, count per workgroup, scan the workgroup totals per item,
//                         give each root its rank: the stream compaction of voxel_common.h, no atomics, so the numbering is by
//                         ascending minimum flat index.
//   label_write_kernel    labels = rank + 1 (+ 1 more for the empty space, whose outside component is label 1).
// Every loop has a hard bound: a find strictly descends, a union strictly lowers one of its two values, and both also stop after
// S^3 rounds.
//   label_stats_*         rows cleared by the call, then integer atomicAdd / atomicMin / atomicMax after a reduction in the wave:
//                         the lanes that share a label are found by ballot, their box follows from the mask, and the first label
//                         a wave meets in its 1024 voxels is merged in registers.
//   topology_*            the labelling twice without the root array (solid 26, empty 6), the roots counted per workgroup, and one
//                         cell-count launch: V, E, F from the row words of the 2 x 2 neighbouring rows with shifts and popc, one
//                         64-bit atomicAdd per workgroup and word.
#include "voxel_common.h"
#include "rn_checks.h"

namespace {

// word w of row (z, y) of the SELECTED set; rows and words outside the grid select nothing, of the empty space either: the
// complement is taken INSIDE the bounds check
template <int S>
__device__ __forceinline__ unsigned sel_word(const unsigned* __restrict__ g, int of_empty, int z, int y, int w)
{
    if (word_outside<S>(z, y, w)) return 0u;
    const unsigned c = occ_word<S>(g, z, y, w);
    return of_empty ? ~c : c;
}

// bits 0..3 = voxels x - 2, x - 1, x, x + 1 of row (z, y) of the selected set
template <int S>
__device__ __forceinline__ unsigned window(const unsigned* __restrict__ g, int of_empty, int z, int y, int x)
{
    const int w = x >> 5;
    const unsigned long long v = ((unsigned long long)sel_word<S>(g, of_empty, z, y, w) << 2) |
                                 (unsigned long long)(sel_word<S>(g, of_empty, z, y, w - 1) >> 30) |
                                 ((unsigned long long)(sel_word<S>(g, of_empty, z, y, w + 1) & 1u) << 34);
    return (unsigned)(v >> (x & 31)) & 15u;
}

template <int S>
__global__ __launch_bounds__(kBlock)
void label_init_kernel(const unsigned* __restrict__ bits, int of_empty, int* __restrict__ parent, int* __restrict__ flag)
{
    constexpr int NW = S / 32, V = S * S * S;
    const int i = blockIdx.x * kBlock + threadIdx.x, x = i % S, row = i / S;
    const unsigned* g = bits + (size_t)blockIdx.y * (V / 32) + row * NW;
    const size_t at = (size_t)blockIdx.y * V + i;
    flag[at] = 0;
    const int wi = x >> 5, bi = x & 31;
    const unsigned own = of_empty ? ~g[wi] : g[wi];
    if (!((own >> bi) & 1u)) { parent[at] = -1; return; }
    unsigned m = ~own & (0xFFFFFFFFu >> (31 - bi));              // unselected voxels at or below x: the nearest ends the run
    int k = wi;
    while (m == 0u && k > 0) { --k; m = of_empty ? g[k] : ~g[k]; }
    parent[at] = row * S + (m != 0u ? k * 32 + 32 - __clz((int)m) : 0);
}

__device__ __forceinline__ int load_parent(int* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int lower_parent(int* p, int v)
{
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of i while other waves unite: parent[i] <= i, so the walk strictly descends; at most `cap` steps
__device__ __forceinline__ int find_shared(int* parent, int i, int cap)
{
    const int from = i;
    int hops = 0;
    for (; hops < cap; ++hops) {
        const int p = load_parent(parent + i);
        if (p >= i || p < 0) break;                              // p == i: a root (anything else cannot be; it ends the walk too)
        i = p;
    }
    if (hops > 1) lower_parent(parent + from, i);                // an ancestor of `from`: shortens later walks
    return i;
}

__device__ __forceinline__ void unite(int* parent, int a, int b, int cap)
{
    for (int round = 0; round < cap; ++round) {
        a = find_shared(parent, a, cap);
        b = find_shared(parent, b, cap);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }            // a is the larger root
        const int old = lower_parent(parent + a, b);
        if (old == a) return;                                    // a was still a root and now hangs below b
        a = old;                                                 // a had a parent already: that one and b remain to be united
    }
}

template <int S>
__global__ __launch_bounds__(kBlock)
void label_merge_kernel(const unsigned* __restrict__ bits, int of_empty, int connectivity, int* __restrict__ parent)
{
    constexpr int V = S * S * S;
    const int i = blockIdx.x * kBlock + threadIdx.x, x = i % S, y = (i / S) % S, z = i / (S * S);
    const unsigned* g = bits + (size_t)blockIdx.y * (V / 32);
    int* par = parent + (size_t)blockIdx.y * V;
    const unsigned own = window<S>(g, of_empty, z, y, x);
    if (!(own & 4u)) return;
    const unsigned own_prev = (own >> 1) & 1u;
    if (connectivity == 6) {
        const int ry[2] = {y - 1, y}, rz[2] = {z, z - 1};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned n = window<S>(g, of_empty, rz[r], ry[r], x);
            if ((n & 4u) && !(own_prev & (n >> 1) & 1u)) unite(par, i, (rz[r] * S + ry[r]) * S + x, V);   // (x - 1, x - 1) joins the same runs
        }
    } else {
        const int ry[4] = {y - 1, y - 1, y, y + 1}, rz[4] = {z, z - 1, z - 1, z - 1};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned n = window<S>(g, of_empty, rz[r], ry[r], x);
            if (n == 0u) continue;
            // the pair (x, p) is left out when (x, p - 1) is a pair (the same run of the neighbour row) or (x - 1, p - 1) is one
            const int at = (rz[r] * S + ry[r]) * S + x;
            if ((n & 2u) && !(own_prev & n & 1u)) unite(par, i, at - 1, V);
            if ((n & 6u) == 4u) unite(par, i, at, V);
            if ((n & 12u) == 8u) unite(par, i, at + 1, V);
        }
    }
}

// kRoots: root[i] = the root of voxel i (-1 unselected).  Without it only the outside flags are set (the topology words).
template <int S, bool kRoots>
__global__ __launch_bounds__(kBlock)
void label_flatten_kernel(const int* __restrict__ parent, int of_empty, int* __restrict__ root, int* __restrict__ flag)
{
    constexpr int V = S * S * S;
    const int i = blockIdx.x * kBlock + threadIdx.x, x = i % S, y = (i / S) % S, z = i / (S * S);
    const int* par = parent + (size_t)blockIdx.y * V;
    const bool border = x == 0 || y == 0 || z == 0 || x == S - 1 || y == S - 1 || z == S - 1;
    if (!kRoots && !of_empty) return;                            // nothing to do (never launched so)
    int r = kRoots || border ? par[i] : -1;
    if (r >= 0) {
        for (int hops = 0; hops < V; ++hops) {
            const int p = par[r];
            if (p >= r || p < 0) break;
            r = p;
        }
    }
    if (kRoots) root[(size_t)blockIdx.y * V + i] = r;
    if (!of_empty) return;
    // one OR per wave and root, and none once the flag is seen set: a border face is thousands of voxels of one component
    const int mark = border ? r : -1;
    unsigned long long todo = __ballot(mark >= 0);
    for (int round = 0; round < kWave && todo != 0ull; ++round) {
        const int first = __ffsll((long long)todo) - 1;
        const int which = __shfl(mark, first);
        todo &= ~__ballot(mark == which);
        if ((int)(threadIdx.x & (kWave - 1)) == first) {
            int* f = flag + (size_t)blockIdx.y * V + which;
            if (!(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1)) atomicOr(f, 1);
        }
    }
}

// a voxel that is the root of a component to be numbered: its own parent, and not joined with the outside
__device__ __forceinline__ bool numbered_root(const int* __restrict__ parent, const int* __restrict__ flag, size_t at, int i)
{
    return parent[at] == i && !(flag[at] & 1);
}

template <int S>
__global__ __launch_bounds__(kBlock)
void label_count_kernel(const int* __restrict__ parent, const int* __restrict__ flag, int* __restrict__ totals)
{
    __shared__ int sw[kWaves];
    constexpr int V = S * S * S;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long roots = __ballot(numbered_root(parent, flag, (size_t)blockIdx.y * V + i, i));
    const int n = block_count<int>(__popcll(roots), sw);
    if (threadIdx.x == 0) totals[(size_t)blockIdx.y * (V / kBlock) + blockIdx.x] = n;
}

// one workgroup per item: exclusive prefixes of the workgroup totals in place, the item's total to counts
__global__ __launch_bounds__(kBlock)
void label_scan_kernel(int* __restrict__ totals, int nb, int* __restrict__ counts)
{
    __shared__ int swave[kWaves];
    const int total = scan_totals(totals + (size_t)blockIdx.x * nb, nb, swave);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// the flag word of a root becomes its rank (0-based), or -1 for a root joined with the outside; other words are never read again
template <int S>
__global__ __launch_bounds__(kBlock)
void label_emit_kernel(const int* __restrict__ parent, int* __restrict__ flag, const int* __restrict__ totals)
{
    __shared__ int sw[kWaves];
    constexpr int V = S * S * S;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const size_t at = (size_t)blockIdx.y * V + i;
    const bool is_root = parent[at] == i, numbered = is_root && !(flag[at] & 1);
    const unsigned long long roots = __ballot(numbered);
    const int rank = totals[(size_t)blockIdx.y * (V / kBlock) + blockIdx.x] + block_rank(__popcll(roots), lanes_before(roots), sw);
    if (is_root) flag[at] = numbered ? rank : -1;
}

template <int S>
__global__ __launch_bounds__(kBlock)
void label_write_kernel(const int* __restrict__ root, const int* __restrict__ rank, int of_empty, int* __restrict__ labels)
{
    constexpr int V = S * S * S;
    const size_t base = (size_t)blockIdx.y * V, at = base + blockIdx.x * kBlock + threadIdx.x;
    const int r = root[at];
    int label = 0;
    if (r >= 0 && r < V) {
        const int k = rank[base + r];
        label = k < 0 ? 1 : k + 1 + (of_empty ? 1 : 0);
    }
    labels[at] = label;
}

// ---- statistics ----

__global__ __launch_bounds__(kBlock)
void label_stats_clear_kernel(const long long* __restrict__ offsets, int B, int S, int* __restrict__ stats)
{
    const long long first = offsets[0], last = offsets[B];
    for (long long r = first + (long long)blockIdx.x * kBlock + threadIdx.x; r < last; r += (long long)gridDim.x * kBlock) {
        int4* row = (int4*)(stats + 8 * r);
        row[0] = make_int4(0, S * S * S, S, S);                  // size, minimum flat index, x_lo, y_lo
        row[1] = make_int4(S, -1, -1, -1);                       // z_lo, x_hi, y_hi, z_hi: the empty box of rn_voxel_pack
    }
}

// what one set of equal labels inside a wave's 64 consecutive voxels adds to its row; every field is wave-uniform
struct Rec { int label, size, first, lo[3], hi[3]; };

// the voxels `m` (bit = lane) of the 64 starting at flat index i0, a multiple of 64: one row or half a row, or two rows at S = 32
template <int S>
__device__ __forceinline__ Rec record_of(unsigned long long m, int i0, int label)
{
    Rec r;
    const int low = __ffsll((long long)m) - 1, high = 63 - __clzll((long long)m);
    r.label = label;
    r.size = __popcll(m);
    r.first = i0 + low;
    const int x0 = i0 % S, y0 = (i0 / S) % S;
    r.lo[2] = r.hi[2] = i0 / (S * S);
    if (S >= 64) {
        r.lo[0] = x0 + low; r.hi[0] = x0 + high;
        r.lo[1] = r.hi[1] = y0;
    } else {
        const unsigned a = (unsigned)m, b = (unsigned)(m >> 32);  // the rows y0 and y0 + 1
        r.lo[0] = min(a ? __ffs((int)a) - 1 : S, b ? __ffs((int)b) - 1 : S);
        r.hi[0] = max(a ? 31 - __clz((int)a) : -1, b ? 31 - __clz((int)b) : -1);
        r.lo[1] = a ? y0 : y0 + 1;
        r.hi[1] = b ? y0 + 1 : y0;
    }
    return r;
}

__device__ __forceinline__ void flush(const Rec& r, long long row0, long long row1, int* __restrict__ stats)
{
    const long long row = row0 + (r.label - 1);
    if (r.label <= 0 || row >= row1) return;                     // a label the offsets have no row for writes nothing
    int* s = stats + 8 * row;
    atomicAdd(s + 0, r.size);
    atomicMin(s + 1, r.first);
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(s + 2 + a, r.lo[a]); atomicMax(s + 5 + a, r.hi[a]); }
}

// A wave walks kStatChunks runs of 64 voxels.  Per run it takes the distinct labels one by one (ballot of the lanes that hold
// the first lane's label: at most 64 rounds); the first label the wave meets is kept in registers and merged there, so a large
// component costs one set of atomics per wave -- per workgroup where its four waves kept the same label -- not per voxel; every
// other label goes to its row at once.
constexpr int kStatChunks = 16;

template <int S>
__global__ __launch_bounds__(kBlock)
void label_stats_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets, int* __restrict__ stats)
{
    constexpr int V = S * S * S;
    const int lane = threadIdx.x & (kWave - 1);
    const int base = (blockIdx.x * kWaves + threadIdx.x / kWave) * (kStatChunks * kWave);
    const int* lab = labels + (size_t)blockIdx.y * V + base + lane;
    const long long row0 = offsets[blockIdx.y], row1 = offsets[blockIdx.y + 1];
    int mine[kStatChunks];
#pragma unroll
    for (int c = 0; c < kStatChunks; ++c) mine[c] = lab[c * kWave];
    Rec kept;
    kept.label = 0;
#pragma unroll
    for (int c = 0; c < kStatChunks; ++c) {
        unsigned long long todo = __ballot(mine[c] > 0);
        for (int round = 0; round < kWave && todo != 0ull; ++round) {
            const int label = __shfl(mine[c], __ffsll((long long)todo) - 1);
            const unsigned long long m = __ballot(mine[c] == label);
            todo &= ~m;
            const Rec r = record_of<S>(m, base + c * kWave, label);
            if (kept.label == 0) {
                kept = r;
            } else if (kept.label == label) {
                kept.size += r.size;                             // r.first is larger: the runs come in ascending order
#pragma unroll
                for (int a = 0; a < 3; ++a) { kept.lo[a] = min(kept.lo[a], r.lo[a]); kept.hi[a] = max(kept.hi[a], r.hi[a]); }
            } else if (lane == 0) {
                flush(r, row0, row1, stats);
            }
        }
    }
    __shared__ Rec waves[kWaves];                                // the four waves' kept labels are often one and the same
    if (lane == 0) waves[threadIdx.x / kWave] = kept;
    __syncthreads();
    if (threadIdx.x != 0) return;
    Rec acc = waves[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        const Rec r = waves[w];
        if (r.label == 0) continue;
        if (acc.label == 0) {
            acc = r;
        } else if (acc.label == r.label) {
            acc.size += r.size;
            acc.first = min(acc.first, r.first);
#pragma unroll
            for (int a = 0; a < 3; ++a) { acc.lo[a] = min(acc.lo[a], r.lo[a]); acc.hi[a] = max(acc.hi[a], r.hi[a]); }
        } else {
            flush(r, row0, row1, stats);
        }
    }
    flush(acc, row0, row1, stats);
}

// ---- topology ----

template <int S>
__global__ __launch_bounds__(kBlock)
void topology_roots_kernel(const int* __restrict__ parent, const int* __restrict__ flag, unsigned long long* __restrict__ words,
                           int word)
{
    __shared__ unsigned long long red[kWaves];
    constexpr int V = S * S * S;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long n = block_sum(numbered_root(parent, flag, (size_t)blockIdx.y * V + i, i) ? 1ull : 0ull, red);
    if (threadIdx.x == 0 && n) atomicAdd(words + (size_t)blockIdx.y * RN_TOPOLOGY_WORDS + word, n);
}

// lattice points 32 w .. 32 w + 31 (and S for the last word) of a row that have a set voxel at x - 1 or x
__device__ __forceinline__ int points(unsigned cur, unsigned prev, bool last_word)
{
    return __popc(cur | (cur << 1) | (prev >> 31)) + (last_word ? (int)(cur >> 31) : 0);
}

// one thread per (lattice zs, lattice ys, word): the rows (zs - 1 | zs, ys - 1 | ys); rows outside the grid are empty
template <int S>
__global__ __launch_bounds__(kBlock)
void topology_cells_kernel(const unsigned* __restrict__ bits, unsigned long long* __restrict__ words)
{
    __shared__ unsigned long long red[kWaves];
    constexpr int NW = S / 32, N = S + 1, V = S * S * S;
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const unsigned* g = bits + (size_t)blockIdx.y * (V / 32);
    unsigned long long n = 0, nv = 0, ne = 0, nf = 0;
    if (k < N * N * NW) {
        const int w = k % NW, y = (k / NW) % N, z = k / (NW * N);
        const bool last = w == NW - 1;
        const unsigned r00 = occ_word<S>(g, z - 1, y - 1, w), r01 = occ_word<S>(g, z - 1, y, w),
                       r10 = occ_word<S>(g, z, y - 1, w), r11 = occ_word<S>(g, z, y, w);
        const unsigned p00 = occ_word<S>(g, z - 1, y - 1, w - 1), p01 = occ_word<S>(g, z - 1, y, w - 1),
                       p10 = occ_word<S>(g, z, y - 1, w - 1), p11 = occ_word<S>(g, z, y, w - 1);
        const unsigned all = r00 | r01 | r10 | r11, pall = p00 | p01 | p10 | p11;
        const unsigned ycell = r01 | r11, pycell = p01 | p11;    // the voxels ys = y under and over lattice zs
        const unsigned zcell = r10 | r11, pzcell = p10 | p11;    // the voxels zs = z before and behind lattice ys
        n = __popc(r11);
        nv = points(all, pall, last);
        ne = __popc(all) + points(ycell, pycell, last) + points(zcell, pzcell, last);     // edges along xs, ys, zs
        nf = points(r11, p11, last) + __popc(zcell) + __popc(ycell);                       // faces across xs, ys, zs
    }
    unsigned long long* out = words + (size_t)blockIdx.y * RN_TOPOLOGY_WORDS;
    const unsigned long long s0 = block_sum(n, red), s3 = block_sum(nv, red), s4 = block_sum(ne, red), s5 = block_sum(nf, red);
    if (threadIdx.x == 0) {
        if (s0) atomicAdd(out + 0, s0);
        if (s3) atomicAdd(out + 3, s3);
        if (s4) atomicAdd(out + 4, s4);
        if (s5) atomicAdd(out + 5, s5);
    }
}

__global__ __launch_bounds__(kBlock)
void topology_finish_kernel(long long* __restrict__ words, int B)
{
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    long long* w = words + (size_t)b * RN_TOPOLOGY_WORDS;
    w[6] = w[3] - w[4] + w[5] - w[0];
    w[7] = w[1] + w[2] - w[6];
}

// ---- host side ----

int check_of_empty(const char* who, int of_empty)
{
    return (of_empty != RN_LABEL_SOLID && of_empty != RN_LABEL_EMPTY)
               ? rn_set_error(RN_E_INVALID, "%s: of_empty=%d (RN_LABEL_SOLID or RN_LABEL_EMPTY)", who, of_empty) : RN_OK;
}

int check_connectivity(const char* who, int connectivity)
{
    return (connectivity != 6 && connectivity != 26) ? rn_set_error(RN_E_INVALID, "%s: connectivity=%d (6 or 26)", who, connectivity)
                                                     : RN_OK;
}

inline size_t voxels(int B, int S) { return (size_t)B * S * S * S; }
inline size_t label_ws_bytes(int B, int S) { return 8 * voxels(B, S) + (voxels(B, S) / kBlock * sizeof(int) + 15) / 16 * 16; }
inline size_t topology_ws_bytes(int B, int S) { return 8 * voxels(B, S); }

// init, merge and flatten: the part the labels and the topology words share
template <int S, bool kRoots>
int launch_forest(const char* who, const unsigned* bits, int B, int of_empty, int connectivity, int* parent, int* root, int* flag,
                  hipStream_t st)
{
    const dim3 grid((unsigned)(S * S * S / kBlock), (unsigned)B), block(kBlock);
    hipLaunchKernelGGL(label_init_kernel<S>, grid, block, 0, st, bits, of_empty, parent, flag);
    hipLaunchKernelGGL(label_merge_kernel<S>, grid, block, 0, st, bits, of_empty, connectivity, parent);
    if (kRoots || of_empty)
        hipLaunchKernelGGL((label_flatten_kernel<S, kRoots>), grid, block, 0, st, (const int*)parent, of_empty, root, flag);
    return rn_check_launch(who);
}

template <int S>
int launch_label(const unsigned* bits, int B, int of_empty, int connectivity, int* labels, int* counts, void* ws, hipStream_t st)
{
    const char* who = "rn_voxel_label";
    constexpr int nb = S * S * S / kBlock;
    int* root = (int*)ws;
    int* flag = root + voxels(B, S);
    int* totals = flag + voxels(B, S);
    int rc = launch_forest<S, true>(who, bits, B, of_empty, connectivity, labels, root, flag, st);
    if (rc != RN_OK) return rc;
    const dim3 grid((unsigned)nb, (unsigned)B), block(kBlock);
    hipLaunchKernelGGL(label_count_kernel<S>, grid, block, 0, st, (const int*)labels, (const int*)flag, totals);
    hipLaunchKernelGGL(label_scan_kernel, dim3((unsigned)B), block, 0, st, totals, nb, counts);
    hipLaunchKernelGGL(label_emit_kernel<S>, grid, block, 0, st, (const int*)labels, flag, (const int*)totals);
    hipLaunchKernelGGL(label_write_kernel<S>, grid, block, 0, st, (const int*)root, (const int*)flag, of_empty, labels);
    return rn_check_launch(who);
}

template <int S>
int launch_topology(const unsigned* bits, int B, long long* out, void* ws, hipStream_t st)
{
    const char* who = "rn_voxel_topology";
    int* parent = (int*)ws;
    int* flag = parent + voxels(B, S);
    unsigned long long* words = (unsigned long long*)out;
    const dim3 grid((unsigned)(S * S * S / kBlock), (unsigned)B), block(kBlock);
    for (int pass = 0; pass < 2; ++pass) {                       // (solid, 26) -> word 1, (empty, 6) -> word 2; the stream orders the reuse
        const int rc = launch_forest<S, false>(who, bits, B, pass, pass ? 6 : 26, parent, (int*)nullptr, flag, st);
        if (rc != RN_OK) return rc;
        hipLaunchKernelGGL(topology_roots_kernel<S>, grid, block, 0, st, (const int*)parent, (const int*)flag, words, 1 + pass);
    }
    constexpr int cells = (S + 1) * (S + 1) * (S / 32);
    hipLaunchKernelGGL(topology_cells_kernel<S>, dim3((unsigned)((cells + kBlock - 1) / kBlock), (unsigned)B), block, 0, st, bits, words);
    hipLaunchKernelGGL(topology_finish_kernel, dim3((unsigned)((B + kBlock - 1) / kBlock)), block, 0, st, out, B);
    return rn_check_launch(who);
}

}  // namespace

extern "C" size_t rn_voxel_label_workspace_bytes(int B, int S)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B)) return 0;
    return label_ws_bytes(B, S);
}

extern "C" int rn_voxel_label(const unsigned* bits, int B, int S, int of_empty, int connectivity, int* labels, int* counts, void* ws,
                              size_t ws_bytes, void* stream)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B) || check_of_empty(__func__, of_empty) ||
        check_connectivity(__func__, connectivity))
        return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(__func__, {bits, labels, counts}) || rn_check_aligned(__func__, bits, 16, "bits") ||
        rn_check_aligned(__func__, labels, 4, "labels") || rn_check_aligned(__func__, counts, 4, "counts") ||
        rn_check_ws(__func__, ws, ws_bytes, label_ws_bytes(B, S)))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (S == 32) return launch_label<32>(bits, B, of_empty, connectivity, labels, counts, ws, st);
    if (S == 64) return launch_label<64>(bits, B, of_empty, connectivity, labels, counts, ws, st);
    return launch_label<128>(bits, B, of_empty, connectivity, labels, counts, ws, st);
}

extern "C" int rn_voxel_label_stats(const int* labels, const long long* offsets, int B, int S, int of_empty, int* stats, void* stream)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B) || check_of_empty(__func__, of_empty)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(__func__, {labels, offsets, stats}) || rn_check_aligned(__func__, labels, 4, "labels") ||
        rn_check_aligned(__func__, offsets, 8, "offsets") || rn_check_aligned(__func__, stats, 16, "stats"))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)(S * S * S / kBlock);
    hipLaunchKernelGGL(label_stats_clear_kernel, dim3(nb < 1024u ? nb : 1024u), dim3(kBlock), 0, st, offsets, B, S, stats);
    const dim3 grid(nb / kStatChunks, (unsigned)B), block(kBlock);
    if (S == 32) hipLaunchKernelGGL(label_stats_kernel<32>, grid, block, 0, st, labels, offsets, stats);
    else if (S == 64) hipLaunchKernelGGL(label_stats_kernel<64>, grid, block, 0, st, labels, offsets, stats);
    else hipLaunchKernelGGL(label_stats_kernel<128>, grid, block, 0, st, labels, offsets, stats);
    return rn_check_launch(__func__);
}

extern "C" size_t rn_voxel_topology_workspace_bytes(int B, int S)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B)) return 0;
    return topology_ws_bytes(B, S);
}

extern "C" int rn_voxel_topology(const unsigned* bits, int B, int S, long long* out_i64, void* ws, size_t ws_bytes, void* stream)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(__func__, {bits, out_i64}) || rn_check_aligned(__func__, bits, 16, "bits") ||
        rn_check_aligned(__func__, out_i64, 8, "out_i64") || rn_check_ws(__func__, ws, ws_bytes, topology_ws_bytes(B, S)))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out_i64, 0, (size_t)B * RN_TOPOLOGY_WORDS * sizeof(long long), st) != hipSuccess)
        return rn_set_error(RN_E_LAUNCH, "%s: clearing the output failed", __func__);
    if (S == 32) return launch_topology<32>(bits, B, out_i64, ws, st);
    if (S == 64) return launch_topology<64>(bits, B, out_i64, ws, st);
    return launch_topology<128>(bits, B, out_i64, ws, st);
}
