// Exact squared Euclidean distance transform of packed occupancy grids, and the shape metrics built on it (gfx950).  Integer
// arithmetic throughout (the one float is the first guess of an integer square root, corrected with integer comparisons); the
// rule is stated in include/rendernet_hip.h (rn_voxel_edt / rn_voxel_shape_metrics), the NumPy twin is tests/voxel_edt_ref.py.
//
// The transform is separable.  Two launches, each a 256-thread block per plane, lanes along xs so that every global and LDS
// access of a wave is a run of consecutive addresses (a uint16 plane read at consecutive xs puts two lanes on each bank's dword:
// no conflict, no padding needed):
//   edt_plane_kernel   block = (zs, item[, direction]).  The seed words of the S rows of the plane go to LDS (occupancy, its
//                      complement, or the surface bits from word shifts with carries and the four neighbouring rows); the row
//                      distance of a voxel is the nearest set bit on each side, found with clz / ffs on masked words; the
//                      min-plus pass along ys runs on the S x S plane in LDS; the two-axis value (<= 2 * 127^2 = 32258, 0xFFFF =
//                      no seed in this plane) leaves as 16 bits.
//   edt_column_kernel  block = (ys, item[, direction]).  Loads the S rows (one per zs) of the intermediate, runs the min-plus
//                      pass along zs, and either writes int32 rows (rn_voxel_edt) or -- rn_voxel_shape_metrics -- keeps the
//                      distance in registers, looks up the OTHER grid's surface bit and reduces: D never reaches memory.
// The min-plus scan walks outwards, delta = 1, 2, ... on both sides, and stops when delta^2 >= best: exact because f >= 0.  A
// missing value is 0xFFFF; a candidate built on it is >= 0x10000, above every finite result (<= 3 * 127^2 = 48387), so it never
// wins and needs no branch.  Whether a position of a line holds a value is the same for every line of a plane (a row or a plane
// has a seed or it has none), so a block finds the first and the last such position once and no walk leaves that range: lines
// through empty space cost nothing.
// Reductions are integer: per block in a fixed order (block_sum, voxel_common.h; block_max here), then one 64-bit vector atomicAdd / atomicMax per block and word into the
// zeroed output, so the result does not depend on arrival order.
#include "voxel_common.h"
#include "rn_checks.h"

namespace {

constexpr unsigned kNone16 = 0xFFFFu;

// occupied voxels with an empty 6-neighbour: bit x of xm / xp is the occupancy of x - 1 / x + 1, carried across the word seam
template <int S>
__device__ __forceinline__ unsigned surf_word(const unsigned* __restrict__ g, int z, int y, int w)
{
    const unsigned c = occ_word<S>(g, z, y, w);
    if (c == 0u) return 0u;
    const unsigned xm = (c << 1) | (occ_word<S>(g, z, y, w - 1) >> 31);
    const unsigned xp = (c >> 1) | (occ_word<S>(g, z, y, w + 1) << 31);
    const unsigned all = xm & xp & occ_word<S>(g, z, y - 1, w) & occ_word<S>(g, z, y + 1, w) & occ_word<S>(g, z - 1, y, w) &
                         occ_word<S>(g, z + 1, y, w);
    return c & ~all;
}

template <int S>
__device__ __forceinline__ unsigned seed_word(const unsigned* __restrict__ g, int seeds, int z, int y, int w)
{
    if (seeds == RN_EDT_SURFACE) return surf_word<S>(g, z, y, w);
    const unsigned c = occ_word<S>(g, z, y, w);
    return seeds == RN_EDT_EMPTY ? ~c : c;                       // complemented AFTER the bounds check: the outside is empty, a seed
}

// distance along xs from voxel x to the nearest set bit of the row's S / 32 words (LDS); 1 << 20 when the row has none
template <int S>
__device__ __forceinline__ int row_distance(const unsigned* row, int x)
{
    constexpr int NW = S / 32;
    const int wi = x >> 5, bi = x & 31;
    int best = 1 << 20;
    unsigned m = row[wi] & (0xFFFFFFFFu >> (31 - bi));          // bits at or below x
    int k = wi;
    while (m == 0u && k > 0) m = row[--k];
    if (m != 0u) best = x - (k * 32 + 31 - __clz((int)m));
    m = row[wi] & (0xFFFFFFFFu << bi);                           // bits at or above x
    k = wi;
    while (m == 0u && k < NW - 1) m = row[++k];
    if (m != 0u) best = min(best, k * 32 + __ffs((int)m) - 1 - x);
    return best;
}

// g(p) = min over p' of f(p') + (p - p')^2 at position p of a line of S values `stride` apart, starting from best = f(p).
// Only positions first..last can hold a value (whether a position holds one is the same for every line of the plane: a row
// has a seed or not), so the walk starts at the nearest of them and ends with the farthest; first > last: none at all.
template <int S>
__device__ __forceinline__ unsigned min_plus(const unsigned short* line, int stride, int p, unsigned best, int first, int last)
{
    if (first > last) return best;
    for (int d = p < first ? first - p : (p > last ? p - last : 1); d < S; ++d) {
        const unsigned dd = (unsigned)(d * d);
        if (dd >= best) break;
        const int lo = p - d, hi = p + d;
        if (lo < first && hi > last) break;
        if (lo >= first) best = min(best, (unsigned)line[lo * stride] + dd);
        if (hi <= last) best = min(best, (unsigned)line[hi * stride] + dd);
    }
    return best;
}

__device__ __forceinline__ unsigned border_sq(int k, int S)     // squared distance to the nearest cell outside the grid
{
    const int b = min(k + 1, S - k);
    return (unsigned)(b * b);
}

template <int S>
__global__ __launch_bounds__(kBlock)
void edt_plane_kernel(const unsigned* __restrict__ bits0, const unsigned* __restrict__ bits1, int seeds,
                      unsigned short* __restrict__ mid)
{
    constexpr int NW = S / 32;
    __shared__ unsigned sw[S * NW];
    __shared__ __attribute__((aligned(16))) unsigned short f[S * S];
    __shared__ int range[2];                                     // first and last row with a seed
    const int t = threadIdx.x, z = blockIdx.x, item = blockIdx.y, dir = blockIdx.z;
    const unsigned* g = (dir ? bits1 : bits0) + (size_t)item * (S * S * NW);
    unsigned short* out = mid + (((size_t)dir * gridDim.y + item) * S + z) * (S * S);

    if (t == 0) { range[0] = S; range[1] = -1; }
    __syncthreads();
    for (int i = t; i < S * NW; i += kBlock) {
        const unsigned w = seed_word<S>(g, seeds, z, i / NW, i % NW);
        sw[i] = w;
        if (w != 0u) { atomicMin(&range[0], i / NW); atomicMax(&range[1], i / NW); }
    }
    __syncthreads();
    const bool empty_rule = seeds == RN_EDT_EMPTY;               // the cells outside the grid are seeds too: never "none"
    const int first = empty_rule ? 0 : range[0], last = empty_rule ? S - 1 : range[1];
    if (first > last) {                                          // uniform over the block
        for (int i = t; i < S * S; i += kBlock) out[i] = (unsigned short)kNone16;
        return;
    }
    for (int i = t; i < S * S; i += kBlock) {
        const int y = i / S, x = i % S;
        int d = row_distance<S>(sw + y * NW, x);
        if (empty_rule) d = min(d, min(x + 1, S - x));
        f[i] = d < S + 1 ? (unsigned short)(d * d) : (unsigned short)kNone16;
    }
    __syncthreads();
    for (int i = t; i < S * S; i += kBlock) {
        const int y = i / S, x = i % S;
        unsigned best = f[i];
        if (empty_rule) best = min(best, border_sq(y, S));
        best = min_plus<S>(f + x, S, y, best, first, last);
        out[i] = (unsigned short)min(best, kNone16);
    }
}

// block_sum's (voxel_common.h) counterpart for a maximum
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned long long a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}

// floor(256 sqrt(D)) = isqrt(D << 16); D <= 3 * 127^2, so D << 16 < 2^32
__device__ __forceinline__ unsigned q_of(unsigned D)
{
    const unsigned long long n = (unsigned long long)D << 16;
    unsigned long long r = (unsigned long long)sqrtf((float)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return (unsigned)r;
}

// kMetrics = false: out_i32 [B,S,S,S] = D (sub = 0) or out - D (sub = 1, the second half of RN_EDT_SIGNED).
// kMetrics = true : direction 0 has the seeds of grid B and is evaluated on the surface of grid A (eval0), direction 1 the converse.
template <int S, bool kMetrics>
__global__ __launch_bounds__(kBlock)
void edt_column_kernel(const unsigned short* __restrict__ mid, int seeds, int sub, int* __restrict__ out_i32,
                       const unsigned* __restrict__ eval0, const unsigned* __restrict__ eval1, unsigned tau2,
                       unsigned long long* __restrict__ words)
{
    constexpr int NW = S / 32;
    __shared__ __attribute__((aligned(16))) unsigned short h[S * S];
    __shared__ unsigned es[kMetrics ? S * NW : 1];
    __shared__ unsigned long long red[4];
    __shared__ int range[2];                                     // first and last zs whose plane has a seed
    const int t = threadIdx.x, y = blockIdx.x, item = blockIdx.y, dir = blockIdx.z;
    const unsigned short* src = mid + (((size_t)dir * gridDim.y + item) * S) * (S * S) + (size_t)y * S;

    if (t == 0) { range[0] = S; range[1] = -1; }
    __syncthreads();
    for (int i = t; i < S * S / 2; i += kBlock) {              // two voxels per lane: rows of S / 2 dwords
        const int z = i / (S / 2), xw = i % (S / 2);
        const unsigned v = ((const unsigned*)(src + (size_t)z * (S * S)))[xw];
        ((unsigned*)h)[i] = v;
        if (xw == 0 && (v & 0xFFFFu) != kNone16) { atomicMin(&range[0], z); atomicMax(&range[1], z); }   // a plane has values everywhere or nowhere
    }
    unsigned long long nA = 0, nB = 0, nAnd = 0, nOr = 0;
    if (kMetrics) {
        const size_t grid_words = (size_t)item * (S * S * NW);
        const unsigned* ga = eval0 + grid_words;
        const unsigned* gb = eval1 + grid_words;
        for (int i = t; i < S * NW; i += kBlock) {
            const int z = i / NW, w = i % NW;
            es[i] = surf_word<S>(dir ? gb : ga, z, y, w);
            if (dir == 0) {
                const unsigned a = occ_word<S>(ga, z, y, w), b = occ_word<S>(gb, z, y, w);
                nA += __popc(a); nB += __popc(b); nAnd += __popc(a & b); nOr += __popc(a | b);
            }
        }
    }
    __syncthreads();
    const bool empty_rule = seeds == RN_EDT_EMPTY;
    const int first = empty_rule ? 0 : range[0], last = empty_rule ? S - 1 : range[1];

    unsigned cnt = 0, sumD = 0, sumQ = 0, maxD = 0, cntTau = 0;  // a thread has S * S / 256 <= 64 voxels: 64 * 56312 < 2^32
    for (int i = t; i < S * S; i += kBlock) {
        const int z = i / S, x = i % S;
        unsigned best = h[i];
        if (empty_rule) best = min(best, border_sq(z, S));
        best = min_plus<S>(h + x, S, z, best, first, last);
        const bool none = best >= kNone16;
        if (!kMetrics) {
            const size_t o = (((size_t)item * S + z) * S + y) * S + x;
            const int D = none ? RN_EDT_NONE : (int)best;
            out_i32[o] = sub ? out_i32[o] - D : D;
        } else if ((es[z * NW + (x >> 5)] >> (x & 31)) & 1u) {
            ++cnt;
            if (!none) {
                sumD += best;
                sumQ += q_of(best);
                maxD = max(maxD, best);
                cntTau += (unsigned)(best <= tau2);
            }
        }
    }
    if (kMetrics) {
        unsigned long long* w = words + (size_t)item * RN_SHAPE_WORDS;
        const unsigned long long r4 = block_sum<unsigned long long>(cnt, red), r6 = block_sum<unsigned long long>(sumD, red),
                                 r8 = block_sum<unsigned long long>(sumQ, red), r12 = block_sum<unsigned long long>(cntTau, red),
                                 r10 = block_max(maxD, red);
        unsigned long long r0 = 0, r1 = 0, r2 = 0, r3 = 0;
        if (dir == 0) {                                          // uniform over the block
            r0 = block_sum(nA, red); r1 = block_sum(nB, red); r2 = block_sum(nAnd, red); r3 = block_sum(nOr, red);
        }
        if (t == 0) {
            if (r0) atomicAdd(w + 0, r0);
            if (r1) atomicAdd(w + 1, r1);
            if (r2) atomicAdd(w + 2, r2);
            if (r3) atomicAdd(w + 3, r3);
            if (r4) atomicAdd(w + 4 + dir, r4);
            if (r6) atomicAdd(w + 6 + dir, r6);
            if (r8) atomicAdd(w + 8 + dir, r8);
            if (r10) atomicMax(w + 10 + dir, r10);
            if (r12) atomicAdd(w + 12 + dir, r12);
        }
    }
}

int check_seeds(const char* who, int seeds)
{
    if (seeds < RN_EDT_SOLID || seeds > RN_EDT_SIGNED)
        return rn_set_error(RN_E_INVALID, "%s: seeds=%d (RN_EDT_SOLID, _EMPTY, _SURFACE or _SIGNED)", who, seeds);
    return RN_OK;
}

inline size_t mid_bytes(int B, int S, int dirs) { return (size_t)dirs * B * S * S * S * sizeof(unsigned short); }

template <int S>
int launch_edt(const unsigned* bits, int B, int seeds, int* out, unsigned short* mid, hipStream_t st)
{
    const dim3 grid((unsigned)S, (unsigned)B, 1u);
    const int first = seeds == RN_EDT_SIGNED ? RN_EDT_SOLID : seeds;
    for (int pass = 0; pass < (seeds == RN_EDT_SIGNED ? 2 : 1); ++pass) {     // the stream orders the second use of `mid`
        const int rule = pass ? RN_EDT_EMPTY : first;
        hipLaunchKernelGGL(edt_plane_kernel<S>, grid, dim3(kBlock), 0, st, bits, bits, rule, mid);
        int rc = rn_check_launch("rn_voxel_edt (plane)");
        if (rc != RN_OK) return rc;
        hipLaunchKernelGGL((edt_column_kernel<S, false>), grid, dim3(kBlock), 0, st, (const unsigned short*)mid, rule, pass, out,
                           (const unsigned*)nullptr, (const unsigned*)nullptr, 0u, (unsigned long long*)nullptr);
        rc = rn_check_launch("rn_voxel_edt (column)");
        if (rc != RN_OK) return rc;
    }
    return RN_OK;
}

template <int S>
int launch_metrics(const unsigned* a, const unsigned* b, int B, unsigned tau2, unsigned long long* words, unsigned short* mid,
                   hipStream_t st)
{
    const dim3 grid((unsigned)S, (unsigned)B, 2u);
    hipLaunchKernelGGL(edt_plane_kernel<S>, grid, dim3(kBlock), 0, st, b, a, RN_EDT_SURFACE, mid);   // direction 0: seeds of B
    const int rc = rn_check_launch("rn_voxel_shape_metrics (plane)");
    if (rc != RN_OK) return rc;
    hipLaunchKernelGGL((edt_column_kernel<S, true>), grid, dim3(kBlock), 0, st, (const unsigned short*)mid, RN_EDT_SURFACE, 0,
                       (int*)nullptr, a, b, tau2, words);
    return rn_check_launch("rn_voxel_shape_metrics (column)");
}

}  // namespace

extern "C" size_t rn_voxel_edt_workspace_bytes(int B, int S, int seeds)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B) || check_seeds(__func__, seeds)) return 0;
    return mid_bytes(B, S, 1);
}

extern "C" int rn_voxel_edt(const unsigned* bits, int B, int S, int seeds, int* out_i32, void* ws, size_t ws_bytes, void* stream)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B) || check_seeds(__func__, seeds)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(__func__, {bits, out_i32}) || rn_check_aligned(__func__, bits, 16, "bits") ||
        rn_check_aligned(__func__, out_i32, 4, "out_i32") || rn_check_ws(__func__, ws, ws_bytes, mid_bytes(B, S, 1)))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    unsigned short* mid = (unsigned short*)ws;
    if (S == 32) return launch_edt<32>(bits, B, seeds, out_i32, mid, st);
    if (S == 64) return launch_edt<64>(bits, B, seeds, out_i32, mid, st);
    return launch_edt<128>(bits, B, seeds, out_i32, mid, st);
}

extern "C" size_t rn_voxel_shape_metrics_workspace_bytes(int B, int S)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B)) return 0;
    return mid_bytes(B, S, 2);
}

extern "C" int rn_voxel_shape_metrics(const unsigned* bits_a, const unsigned* bits_b, int B, int S, int tau2, long long* out_i64,
                                      void* ws, size_t ws_bytes, void* stream)
{
    if (rn_check_grid_side_pow2(__func__, S) || rn_check_batch(__func__, B)) return RN_E_INVALID;
    if (tau2 < 0) return rn_set_error(RN_E_INVALID, "%s: tau2=%d (floor(tau^2) >= 0)", __func__, tau2);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(__func__, {bits_a, bits_b, out_i64}) || rn_check_aligned(__func__, bits_a, 16, "bits_a") ||
        rn_check_aligned(__func__, bits_b, 16, "bits_b") || rn_check_aligned(__func__, out_i64, 8, "out_i64") ||
        rn_check_ws(__func__, ws, ws_bytes, mid_bytes(B, S, 2)))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out_i64, 0, (size_t)B * RN_SHAPE_WORDS * sizeof(long long), st) != hipSuccess)
        return rn_set_error(RN_E_LAUNCH, "%s: clearing the output failed", __func__);
    unsigned short* mid = (unsigned short*)ws;
    unsigned long long* words = (unsigned long long*)out_i64;
    if (S == 32) return launch_metrics<32>(bits_a, bits_b, B, (unsigned)tau2, words, mid, st);
    if (S == 64) return launch_metrics<64>(bits_a, bits_b, B, (unsigned)tau2, words, mid, st);
    return launch_metrics<128>(bits_a, bits_b, B, (unsigned)tau2, words, mid, st);
}
