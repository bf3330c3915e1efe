// Voxel registration: the signed axis permutation and integer shift of grid A that overlaps grid B most (gfx950).  The rule -- the
// numbering of the 48 orientations, a candidate (o, t), its score n_and, the tie order, the limits -- is stated in
// include/rendernet_hip.h (rn_voxel_orient, rn_voxel_align); the NumPy twin is tests/voxel_align_ref.py.  Integers only.
//
//   orient_kernel       thread = one word of one oriented copy.  An orientation that keeps x on x copies the source word, or
//                       reverses it (__brev) and swaps the words of the row; the others gather 32 bits that sit at one bit
//                       position of 32 source words.  No atomics: every output word has one writer.
//   correlate_kernel    workgroup = (tz, orientation, pair).  B's rows live in registers, a lane holding kRows rows of W words;
//                       the oriented A, moved by tz, is staged in LDS by z-slabs of at most 32 KB (the whole grid up to 64^3,
//                       16 planes of 128^3), rows outside the grid as zeros.  For every ty a lane reads the A row that meets
//                       each of its B rows and walks all tx in registers: v_alignbit across the words of the row, &, popcount.
//                       A loaded word serves 2 RT + 1 candidates; a wave skips a round in which its 64 rows of B are all
//                       empty.  The sums of a ty are added over the wave by a butterfly of shuffles (Fold) that leaves each
//                       with one lane, and go into a table in LDS by one integer add each; the table is stored when the slabs
//                       are done.  RT is R rounded up to 4, 8 or 16: the shifts are compile-time constants, and the sums
//                       beyond R are computed and dropped.  Integer adds commute, so the table is a function of the bits
//                       alone.  The workgroup also leaves the largest 64-bit key of its (2R+1)^2 candidates, the key holding
//                       n_and and the tie order in descending fields.
//   winner_kernel       workgroup = pair: the largest of the pair's keys, one per correlate workgroup, and the popcounts of A
//                       and B.  The maximum of a set does not depend on the order it is taken in.
#include "voxel_common.h"
#include "rn_checks.h"

namespace {

constexpr int kMaxShift = RN_ALIGN_MAX_SHIFT;
constexpr int kOrientations = 48;
constexpr int kSlabBytes = 32768;
constexpr int kSetSizes[3] = {1, 24, 48};

// orientation o as pi(0) | pi(1) << 2 | pi(2) << 4 | f0 << 6 | f1 << 7 | f2 << 8
struct OrientTable { unsigned short code[kOrientations]; };

OrientTable orient_table()
{
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};   // lexicographic
    static const int odd[6] = {0, 1, 1, 0, 0, 1};
    OrientTable t;
    int n[2] = {0, 24};
    for (int p = 0; p < 6; ++p)
        for (int f = 0; f < 8; ++f) {                              // (f0, f1, f2) lexicographic: f0 is the high bit
            const int f0 = (f >> 2) & 1, f1 = (f >> 1) & 1, f2 = f & 1;
            const int mirrored = (odd[p] + f0 + f1 + f2) & 1;
            t.code[n[mirrored]++] = (unsigned short)(perms[p][0] | perms[p][1] << 2 | perms[p][2] << 4 | f0 << 6 | f1 << 7 | f2 << 8);
        }
    return t;
}

// ---- orient ---------------------------------------------------------------------------------------------------------------------

template <int S>
__device__ __forceinline__ int axis_stride(int axis) { return axis == 0 ? S * S : (axis == 1 ? S : 1); }

template <int S>
__global__ __launch_bounds__(kBlock)
void orient_kernel(const unsigned* __restrict__ in, unsigned* __restrict__ out, OrientTable table, int o_first, int o_count)
{
    constexpr int W = S / 32, kWords = S * S * W;
    const int idx = blockIdx.x * kBlock + threadIdx.x;            // kWords is a multiple of kBlock
    const int oi = blockIdx.y, b = blockIdx.z;
    const int code = table.code[o_first + oi];
    const int p0 = code & 3, p1 = (code >> 2) & 3, p2 = (code >> 4) & 3;
    const int f0 = (code >> 6) & 1, f1 = (code >> 7) & 1, f2 = (code >> 8) & 1;
    const int w = idx % W, y = (idx / W) % S, z = idx / (W * S);
    const unsigned* __restrict__ g = in + (size_t)b * kWords;
    // source voxel j with j[pi(k)] = the output index on axis k, flipped where f_k is set; its flat index is the sum of j[a] * stride(a)
    const int base = (f0 ? S - 1 - z : z) * axis_stride<S>(p0) + (f1 ? S - 1 - y : y) * axis_stride<S>(p1);
    unsigned word;
    if (p2 == 2) {                                                // x stays x: the row is a row of the source (base is a multiple of S)
        const unsigned* row = g + base / 32;
        word = f2 ? __brev(row[W - 1 - w]) : row[w];
    } else {
        word = 0u;
        const int stride = axis_stride<S>(p2);                    // bits of the source between two steps of the output x
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const int x = 32 * w + k;
            const int i = base + (f2 ? S - 1 - x : x) * stride;   // < S^3: a sum of three coordinates below S, each times its stride
            word |= ((g[i >> 5] >> (i & 31)) & 1u) << k;
        }
    }
    out[((size_t)b * o_count + oi) * kWords + idx] = word;
}

// ---- correlate ------------------------------------------------------------------------------------------------------------------

template <int W> struct Row { unsigned w[W]; };

template <int S>
struct Slab {
    static constexpr int W = S / 32;
    static constexpr int kPlanes = (S * S * W * 4 <= kSlabBytes) ? S : kSlabBytes / (S * W * 4);
    static constexpr int kWords = kPlanes * S * W;
    static constexpr int kRows = kPlanes * S / kBlock;            // B rows a lane holds
    static_assert(S % kPlanes == 0 && (kPlanes * S) % kBlock == 0 && kRows <= 32, "a slab is whole planes and at most 32 whole rounds of the workgroup");
};

// word w of the row moved by TX: bit x of the result is bit x - TX of the row, zeros entering at either end
template <int W, int TX>
__device__ __forceinline__ unsigned moved_word(const Row<W>& a, int w)
{
    if (TX == 0) return a.w[w];
    if (TX > 0) return __funnelshift_l(w > 0 ? a.w[w - 1] : 0u, a.w[w], TX);
    return __funnelshift_r(a.w[w], w + 1 < W ? a.w[w + 1] : 0u, -TX);
}

template <int W, int RT, int K>
struct Walk {                                                     // acc[K] += |moved(a, K - RT) & b| for K .. 2 RT
    static __device__ __forceinline__ void run(const Row<W>& a, const Row<W>& b, int* acc)
    {
#pragma unroll
        for (int w = 0; w < W; ++w) acc[K] += __popc(moved_word<W, K - RT>(a, w) & b.w[w]);
        Walk<W, RT, K + 1>::run(a, b, acc);
    }
};
template <int W, int RT>
struct Walk<W, RT, 2 * RT + 1> {
    static __device__ __forceinline__ void run(const Row<W>&, const Row<W>&, int*) {}
};

// n_and (22 bits) | 1023 - |t|^2 | 63 - o | 16 - tz | 16 - ty | 16 - tx: the largest key is the winner of the tie order
__device__ __forceinline__ unsigned long long candidate_key(int n_and, int o, int tz, int ty, int tx)
{
    const int t2 = tz * tz + ty * ty + tx * tx;                   // <= 768
    return ((unsigned long long)n_and << 34) | ((unsigned long long)(1023 - t2) << 24) | ((unsigned long long)(63 - o) << 18) |
           ((unsigned long long)(kMaxShift - tz) << 12) | ((unsigned long long)(kMaxShift - ty) << 6) |
           (unsigned long long)(kMaxShift - tx);
}

// the largest key of the workgroup, in thread 0; `sk` is kWaves words of LDS.  Every thread calls it: it holds a barrier
__device__ __forceinline__ unsigned long long block_max_key(unsigned long long key, unsigned long long* sk)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long k = __shfl_down(key, off, 64);
        key = k > key ? k : key;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) sk[threadIdx.x / kWave] = key;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kWaves; ++j) key = sk[j] > key ? sk[j] : key;
    return key;
}

// The sums of N values over the 64 lanes of a wave in about N + 4 shuffles instead of 6 N (21 for N = 17): a butterfly in which
// the two lanes of a pair (lane ^ D) split the values between them -- the lane with bit D clear sums the lower half ceil(N/2),
// the other the upper half, a missing value counting as zero -- and go on with half as many at D / 2.  After D = 1 a lane holds in v[0] the sum over
// the wave of the value of index k (k is advanced by the halves the lane left behind), or zero: the sum of every index below N
// sits in exactly one lane, and a lane that ends on an index without a value (k >= N, or the upper lane of a pair that had one
// value left) holds zero.  Integer adds: the order does not show.
template <int N, int D>
struct Fold {
    static __device__ __forceinline__ void run(int* v, int lane, int& k)
    {
        constexpr int H = (N + 1) / 2;
        const bool up = (lane & D) != 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const int lo = v[i], hi = H + i < N ? v[H + i] : 0;
            v[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, D, 64);
        }
        k += up ? H : 0;
        Fold<H, D / 2>::run(v, lane, k);
    }
};
template <int N>
struct Fold<N, 0> {
    static __device__ __forceinline__ void run(int*, int, int&) { static_assert(N == 1, "six halvings take up to 64 values to one"); }
};

template <int S, int RT>
__global__ __launch_bounds__(kBlock)
void correlate_kernel(const unsigned* __restrict__ oriented, const unsigned* __restrict__ bits_b, int* __restrict__ scores,
                      unsigned long long* __restrict__ keys, int R, int n_orient)
{
    using SL = Slab<S>;
    constexpr int W = SL::W, kGrid = S * S * W;
    __shared__ __attribute__((aligned(16))) unsigned sa[SL::kWords];
    __shared__ int tab[(2 * kMaxShift + 1) * (2 * kMaxShift + 1)];
    __shared__ unsigned long long skey[kWaves];
    const int T = 2 * R + 1;
    const int tz = (int)blockIdx.x - R, oi = blockIdx.y, b = blockIdx.z;
    const unsigned* __restrict__ ga = oriented + ((size_t)b * n_orient + oi) * kGrid;
    const unsigned* __restrict__ gb = bits_b + (size_t)b * kGrid;
    const int t = threadIdx.x, lane = t & (kWave - 1);
    for (int i = t; i < T * T; i += kBlock) tab[i] = 0;

    for (int z0 = 0; z0 < S; z0 += SL::kPlanes) {
        __syncthreads();                                          // the previous slab is read to its end (and tab is cleared)
        for (int i = 4 * t; i < SL::kWords; i += 4 * kBlock) {    // A'(z) = A(z - tz): plane z0 + zl of the slab is A's z0 + zl - tz
            const int za = z0 + i / (S * W) - tz;                 // four words of one plane: S W is a multiple of 4
            *(uint4*)(sa + i) = (unsigned)za < (unsigned)S ? *(const uint4*)(ga + za * (S * W) + i % (S * W)) : make_uint4(0u, 0u, 0u, 0u);
        }
        Row<W> rb[SL::kRows];
        unsigned live = 0u;                                       // kRows <= 32
#pragma unroll
        for (int j = 0; j < SL::kRows; ++j) {                     // row j kBlock + t of the slab: consecutive lanes, consecutive ys
            const int r = j * kBlock + t;
#pragma unroll
            for (int w = 0; w < W; ++w) rb[j].w[w] = gb[(z0 * S + r) * W + w];
            unsigned any = 0u;
#pragma unroll
            for (int w = 0; w < W; ++w) any |= rb[j].w[w];
            live |= (__ballot(any != 0u) != 0ull ? 1u : 0u) << j;  // uniform: does any of the wave's 64 rows of round j hold a voxel
        }
        __syncthreads();
        for (int ty = -R; ty <= R; ++ty) {
            int acc[2 * RT + 1];
#pragma unroll
            for (int k = 0; k <= 2 * RT; ++k) acc[k] = 0;
#pragma unroll
            for (int j = 0; j < SL::kRows; ++j) {
                if (!((live >> j) & 1u)) continue;                // 64 empty rows of B add nothing to any sum: the wave skips them
                const int r = j * kBlock + t;
                const int ya = r % S - ty;                        // A'(y) = A(y - ty)
                Row<W> ra;
                const bool in = (unsigned)ya < (unsigned)S;
                const int at = in ? ((r / S) * S + ya) * W : 0;   // inside the slab either way
#pragma unroll
                for (int w = 0; w < W; ++w) ra.w[w] = in ? sa[at + w] : 0u;
                Walk<W, RT, 0>::run(ra, rb[j], acc);
            }
            int k = 0;                                            // the sums of the wave: lane's acc[0] is that of shift k - RT
            Fold<2 * RT + 1, 32>::run(acc, lane, k);
            const int tx = k - RT;
            if (tx >= -R && tx <= R && acc[0] != 0) atomicAdd(&tab[(ty + R) * T + tx + R], acc[0]);   // the sums beyond R are dropped
        }
    }
    __syncthreads();
    int* __restrict__ out = scores + (((size_t)b * n_orient + oi) * T + (tz + R)) * (size_t)(T * T);
    unsigned long long key = 0ull;                                // below every candidate's: 1023 - |t|^2 > 0
    for (int i = t; i < T * T; i += kBlock) {
        out[i] = tab[i];
        const unsigned long long k = candidate_key(tab[i], oi, tz, i / T - R, i % T - R);
        key = k > key ? k : key;
    }
    key = block_max_key(key, skey);
    if (t == 0) keys[((size_t)b * n_orient + oi) * T + (tz + R)] = key;    // the best of this workgroup's (2R+1)^2 candidates
}

// ---- winner ---------------------------------------------------------------------------------------------------------------------

template <int S>
__global__ __launch_bounds__(kBlock)
void winner_kernel(const unsigned* __restrict__ bits_a, const unsigned* __restrict__ bits_b, const int* __restrict__ scores,
                   const unsigned long long* __restrict__ keys, int* __restrict__ best, int R, int n_orient)
{
    constexpr int kGrid = S * S * S / 32;
    __shared__ unsigned long long skey[kWaves];
    __shared__ int red[kWaves];
    const int b = blockIdx.x, t = threadIdx.x, T = 2 * R + 1;
    const int n = n_orient * T;                                   // one key per correlate workgroup of the pair
    unsigned long long key = 0ull;
    for (int i = t; i < n; i += kBlock) {
        const unsigned long long k = keys[(size_t)b * n + i];
        key = k > key ? k : key;
    }
    key = block_max_key(key, skey);
    int na = 0, nb = 0;
    for (int i = t; i < kGrid; i += kBlock) {
        na += __popc(bits_a[(size_t)b * kGrid + i]);
        nb += __popc(bits_b[(size_t)b * kGrid + i]);
    }
    na = block_sum(na, red);
    nb = block_sum(nb, red);
    if (t == 0) {
        int* w = best + (size_t)b * 8;
        w[0] = 63 - (int)((key >> 18) & 63);
        w[1] = kMaxShift - (int)((key >> 12) & 63);
        w[2] = kMaxShift - (int)((key >> 6) & 63);
        w[3] = kMaxShift - (int)(key & 63);
        w[4] = (int)(key >> 34);
        w[5] = na;
        w[6] = nb;
        w[7] = scores[(size_t)b * n * (T * T) + (R * T + R) * T + R];    // orientation 0 is the first of every set
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------------------

template <int S>
void launch_orient(const unsigned* in, unsigned* out, int B, int o_first, int o_count, hipStream_t st)
{
    static const OrientTable table = orient_table();
    hipLaunchKernelGGL(orient_kernel<S>, dim3((unsigned)(S * S * (S / 32) / kBlock), (unsigned)o_count, (unsigned)B), dim3(kBlock),
                       0, st, in, out, table, o_first, o_count);
}

template <int S>
void launch_correlate(const unsigned* oriented, const unsigned* bits_b, int* scores, unsigned long long* keys, int B, int R,
                      int n_orient, hipStream_t st)
{
    const dim3 grid((unsigned)(2 * R + 1), (unsigned)n_orient, (unsigned)B);
    if (R <= 4) hipLaunchKernelGGL((correlate_kernel<S, 4>), grid, dim3(kBlock), 0, st, oriented, bits_b, scores, keys, R, n_orient);
    else if (R <= 8) hipLaunchKernelGGL((correlate_kernel<S, 8>), grid, dim3(kBlock), 0, st, oriented, bits_b, scores, keys, R, n_orient);
    else hipLaunchKernelGGL((correlate_kernel<S, 16>), grid, dim3(kBlock), 0, st, oriented, bits_b, scores, keys, R, n_orient);
}

template <int S>
void launch_align(const unsigned* bits_a, const unsigned* bits_b, unsigned* oriented, int* scores, unsigned long long* keys,
                  int* best, int B, int R, int n_orient, hipStream_t st)
{
    launch_orient<S>(bits_a, oriented, B, 0, n_orient, st);
    launch_correlate<S>(oriented, bits_b, scores, keys, B, R, n_orient, st);
    hipLaunchKernelGGL(winner_kernel<S>, dim3((unsigned)B), dim3(kBlock), 0, st, bits_a, bits_b, scores, keys, best, R, n_orient);
}

size_t oriented_bytes(int B, int S, int n_orient) { return (size_t)B * n_orient * ((size_t)S * S * S / 8); }

size_t keys_bytes(int B, int R, int n_orient) { return (size_t)B * n_orient * (2 * (size_t)R + 1) * sizeof(unsigned long long); }

size_t table_bytes(int B, int R, int n_orient)
{
    const size_t T = 2 * (size_t)R + 1;
    return (size_t)B * n_orient * T * T * T * sizeof(int);
}

int check_search(const char* what, int R, int orient_set)
{
    if (R < 0 || R > kMaxShift) return rn_set_error(RN_E_INVALID, "%s: R=%d (0..%d)", what, R, kMaxShift);
    if (orient_set < RN_ALIGN_NONE || orient_set > RN_ALIGN_ALL)
        return rn_set_error(RN_E_INVALID, "%s: orient_set=%d (0 none, 1 rotations, 2 all)", what, orient_set);
    return RN_OK;
}

}  // namespace

extern "C" int rn_voxel_orient(const unsigned* bits_in, int B, int S, int o_first, int o_count, unsigned* bits_out, void* stream)
{
    const char* what = __func__;
    if (rn_check_grid_side_pow2(what, S) || rn_check_batch(what, B)) return RN_E_INVALID;
    if (o_first < 0 || o_count < 0 || o_first > kOrientations - o_count)
        return rn_set_error(RN_E_INVALID, "%s: orientations %d .. %d + %d (inside 0..%d)", what, o_first, o_first, o_count, kOrientations - 1);
    if (B == 0 || o_count == 0) return RN_OK;
    if (rn_check_pointers(what, {bits_in, bits_out}) || rn_check_aligned(what, bits_in, 4, "bits_in") ||
        rn_check_aligned(what, bits_out, 4, "bits_out"))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (S == 32) launch_orient<32>(bits_in, bits_out, B, o_first, o_count, st);
    else if (S == 64) launch_orient<64>(bits_in, bits_out, B, o_first, o_count, st);
    else launch_orient<128>(bits_in, bits_out, B, o_first, o_count, st);
    return rn_check_launch(what);
}

extern "C" size_t rn_voxel_align_workspace_bytes(int B, int S, int R, int n_orient)
{
    if ((S != 32 && S != 64 && S != 128) || B < 0 || B > kMaxBatch || R < 0 || R > kMaxShift || n_orient < 1 || n_orient > kOrientations)
        return 0;
    return oriented_bytes(B, S, n_orient) + keys_bytes(B, R, n_orient) + table_bytes(B, R, n_orient);   // in this order, each 8-byte aligned
}

extern "C" int rn_voxel_align(const unsigned* bits_a, const unsigned* bits_b, int B, int S, int R, int orient_set, int* out_best,
                              int* out_scores, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* what = __func__;
    if (rn_check_grid_side_pow2(what, S) || rn_check_batch(what, B) || check_search(what, R, orient_set)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    const int n_orient = kSetSizes[orient_set];
    if (rn_check_pointers(what, {bits_a, bits_b, out_best}) || rn_check_aligned(what, bits_a, 4, "bits_a") ||
        rn_check_aligned(what, bits_b, 4, "bits_b") || rn_check_aligned(what, out_best, 4, "out_best") ||
        rn_check_aligned(what, out_scores, 4, "out_scores") ||
        rn_check_ws(what, workspace, workspace_bytes, rn_voxel_align_workspace_bytes(B, S, R, n_orient)))
        return RN_E_INVALID;
    unsigned* oriented = (unsigned*)workspace;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + oriented_bytes(B, S, n_orient));
    int* scores = out_scores ? out_scores : (int*)((char*)keys + keys_bytes(B, R, n_orient));
    hipStream_t st = (hipStream_t)stream;
    if (S == 32) launch_align<32>(bits_a, bits_b, oriented, scores, keys, out_best, B, R, n_orient, st);
    else if (S == 64) launch_align<64>(bits_a, bits_b, oriented, scores, keys, out_best, B, R, n_orient, st);
    else launch_align<128>(bits_a, bits_b, oriented, scores, keys, out_best, B, R, n_orient, st);
    return rn_check_launch(what);
}
