// Silhouette pose search: one silhouette scored against a grid under thousands of candidate cameras (gfx950).  The rule -- the
// pixel a voxel's centre falls into, the footprint, the two counts of a candidate, the order of two candidates, the limits and
// the bounds -- is stated in include/rendernet_hip.h (rn_mask_pack, rn_pose_score, rn_pose_best); the NumPy twin is
// tests/voxel_pose_ref.py.  Integers only.
//
//   mask_pack_kernel    workgroup = item: a thread builds one word of 32 pixels of a row at a time; the foreground count is the
//                       fixed-order block_sum of the popcounts.
//   pose_score_kernel   workgroup = (candidate, item).  The splat image is bits in LDS, ph rows of ceil(pw / 32) words, at most
//                       8 KB, cleared by the workgroup and set with LDS atomicOr: an OR commutes, so the image does not depend on
//                       the order the voxels arrive in, there are no global atomics and nothing to clear between calls.  The
//                       camera's address depends on blockIdx only, so its eight words come through the scalar data cache.  A
//                       lane takes a row word of 32 voxels along xs -- from the list of the item's occupied words that
//                       pose_words_kernel leaves in the workspace, or, without a workspace, walking every word and skipping
//                       the zero ones; DESIGN.md 5c has the timing of both -- and forms the affine value of the
//                       word's first centre once (two rows) and adds 256 a_x times the bit index for every set bit -- exact in
//                       int64, the same integer as the full a . q + b -- and finishes with mesh_project.h's rounding shift and
//                       clamps.  After a barrier the workgroup popcounts splat and splat & mask word by word (block_sum) and,
//                       when the caller wants them, stores the splat as bytes.
//   pose_best_kernel    workgroup = item: every thread keeps the best of its candidates p = t, t + 256, ..., then the waves and
//                       the workgroup keep the best of theirs.  The order is total (the cross-multiplied quotients, then the
//                       lower index), so the maximum does not depend on the order it is taken in.
#include "voxel_common.h"
#include "rn_checks.h"
#include "mesh_project.h"

namespace {

constexpr int kMaxSide = 256;                            // ph, pw: the splat image is at most 256 rows of 8 words
constexpr int kMaxImageWords = kMaxSide * (kMaxSide / 32);
constexpr int kMaxPoses = 65535;                         // blockIdx.x carries the candidate
constexpr int kMaxFootprint = 4;

__global__ __launch_bounds__(kBlock)
void mask_pack_kernel(const unsigned char* __restrict__ mask, unsigned* __restrict__ mask_bits, int* __restrict__ n_mask, int ph, int pw)
{
    __shared__ int red[kWaves];
    const int b = blockIdx.x, IW = (pw + 31) / 32;
    const unsigned char* __restrict__ m = mask + (size_t)b * ph * pw;
    int n = 0;
    for (int i = threadIdx.x; i < ph * IW; i += kBlock) {
        const int r = i / IW, c0 = 32 * (i % IW);
        unsigned word = 0u;
        for (int k = 0; k < 32 && c0 + k < pw; ++k) word |= (m[r * pw + c0 + k] != 0 ? 1u : 0u) << k;   // bits past pw stay 0
        mask_bits[(size_t)b * ph * IW + i] = word;
        n += __popc(word);
    }
    n = block_sum(n, red);
    if (threadIdx.x == 0) n_mask[b] = n;
}

// The occupied words of every item, listed once for the P workgroups that would each walk them: words[b][0 .. counts[b]) are the
// indices of the nonzero row words of grid b in rising order.  Workgroup = item, 256 words a round; a word's place is the total
// of the rounds before plus block_rank of voxel_common.h: no atomics, so the list is a function of the bits alone (the scores
// would be the same in any order of it: an OR commutes).
__global__ __launch_bounds__(kBlock)
void pose_words_kernel(const unsigned* __restrict__ bits, int* __restrict__ words, int* __restrict__ counts, int n_words)
{
    __shared__ int sw[kWaves];
    const int b = blockIdx.x, t = threadIdx.x;
    const unsigned* __restrict__ g = bits + (size_t)b * n_words;
    int* __restrict__ out = words + (size_t)b * n_words;
    int base = 0;
    for (int i0 = 0; i0 < n_words; i0 += kBlock) {                 // n_words = S^3 / 32 is a multiple of kBlock
        const int i = i0 + t;
        const bool on = g[i] != 0u;
        const unsigned long long vote = __ballot(on);
        __syncthreads();                                           // sw is still read from the round before
        const int rank = block_rank(__popcll(vote), lanes_before(vote), sw);
        if (on) out[base + rank] = i;                              // base + rank < the words seen so far <= n_words
        base += ((sw[0] + sw[1]) + sw[2]) + sw[3];
    }
    if (t == 0) counts[b] = base;
}

// kList: visit words[b][0 .. counts[b]), the list pose_words_kernel left; otherwise walk every word and skip the zero ones
template <bool kList>
__global__ __launch_bounds__(kBlock)
void pose_score_kernel(const unsigned* __restrict__ bits, const unsigned* __restrict__ mask_bits, const i64* __restrict__ cam,
                       const int* __restrict__ words, const int* __restrict__ counts, int* __restrict__ scores,
                       unsigned char* __restrict__ splats, int P, int S, int row0, int col0, int ph, int pw, int fp)
{
    __shared__ unsigned img[kMaxImageWords];
    __shared__ int red[kWaves];
    const int p = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int W = S / 32, n_words = S * S * W, IW = (pw + 31) / 32, n_img = ph * IW;      // n_img <= kMaxImageWords: ph, pw <= 256
    for (int i = t; i < n_img; i += kBlock) img[i] = 0u;
    __syncthreads();

    const i64* __restrict__ c = cam + ((size_t)b * P + p) * 12;                            // uniform address; rows 0 and 1 only
    const i64 step_x = 256 * c[2], step_y = 256 * c[6];                                    // one voxel along xs
    const i64 lead = 128 * (fp - 1);                                                       // the footprint's lead over the centre
    const unsigned* __restrict__ g = bits + (size_t)b * n_words;
    const int* __restrict__ list = kList ? words + (size_t)b * n_words : nullptr;
    const int n_visit = kList ? counts[b] : n_words;               // counts[b] <= n_words, every listed index < n_words
    for (int j = t; j < n_visit; j += kBlock) {
        const int i = kList ? list[j] : j;
        unsigned word = g[i];
        if (!kList && word == 0u) continue;
        const int w = i % W, y = (i / W) % S, z = i / (W * S);
        const i64 q0 = 256 * z + 128, q1 = 256 * y + 128, q2 = 256 * (32 * w) + 128;      // the centre of the word's first voxel
        const i64 sx = c[0] * q0 + c[1] * q1 + c[2] * q2 + c[3];
        const i64 sy = c[4] * q0 + c[5] * q1 + c[6] * q2 + c[7];
        while (word != 0u) {
            const int k = __ffs((int)word) - 1;
            word &= word - 1u;
            const i64 X = project_finish(sx + step_x * k, 0), Y = project_finish(sy + step_y * k, 1);
            const int pr = (int)((Y - lead) >> 8) - row0, pc = (int)((X - lead) >> 8) - col0;   // floor: |X|, |Y| <= 2^20
            for (int di = 0; di < fp; ++di) {
                const int r = pr + di;
                if ((unsigned)r >= (unsigned)ph) continue;
                for (int dj = 0; dj < fp; ++dj) {
                    const int cc = pc + dj;
                    if ((unsigned)cc < (unsigned)pw) atomicOr(&img[r * IW + (cc >> 5)], 1u << (cc & 31));   // r < ph, cc >> 5 < IW
                }
            }
        }
    }
    __syncthreads();

    const unsigned* __restrict__ mb = mask_bits + (size_t)b * n_img;
    int n_splat = 0, n_inter = 0;
    for (int i = t; i < n_img; i += kBlock) {
        const unsigned s = img[i];
        n_splat += __popc(s);
        n_inter += __popc(s & mb[i]);
    }
    n_splat = block_sum(n_splat, red);
    n_inter = block_sum(n_inter, red);
    const size_t item = (size_t)b * P + p;
    if (t == 0) {
        scores[2 * item] = n_splat;
        scores[2 * item + 1] = n_inter;
    }
    if (splats) {
        unsigned char* __restrict__ out = splats + item * ((size_t)ph * pw);
        for (int i = t; i < ph * pw; i += kBlock) {
            const int r = i / pw, cc = i % pw;
            out[i] = (unsigned char)((img[r * IW + (cc >> 5)] >> (cc & 31)) & 1u);
        }
    }
}

struct Cand { int n_inter, n_union, index; };             // n_union >= 1

__device__ __forceinline__ Cand candidate(const int* __restrict__ s, int n_mask, int p)
{
    const int n_union = s[2 * p] + n_mask - s[2 * p + 1];
    return {n_union > 0 ? s[2 * p + 1] : 0, n_union > 0 ? n_union : 1, p};                // a union of 0 counts as 0 / 1
}

// a beats b: the larger n_inter / n_union by cross-multiplication, equal quotients to the lower index
__device__ __forceinline__ bool beats(const Cand& a, const Cand& b)
{
    const i64 l = (i64)a.n_inter * b.n_union, r = (i64)b.n_inter * a.n_union;            // |.| <= 2^16 * 2^17
    return l > r || (l == r && a.index < b.index);
}

__global__ __launch_bounds__(kBlock)
void pose_best_kernel(const int* __restrict__ scores, const int* __restrict__ n_mask, int* __restrict__ best,
                      int* __restrict__ best_counts, int P)
{
    __shared__ Cand sc[kWaves];
    const int b = blockIdx.x, t = threadIdx.x, nm = n_mask[b];
    const int* __restrict__ s = scores + (size_t)b * P * 2;
    Cand mine = candidate(s, nm, t < P ? t : P - 1);              // P >= 1; a thread past the end holds a copy of the last one,
    for (int p = t + kBlock; p < P; p += kBlock) {                //   which beats nothing it ties with: every index kept is < P
        const Cand c = candidate(s, nm, p);
        if (beats(c, mine)) mine = c;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const Cand o = {__shfl_down(mine.n_inter, off, 64), __shfl_down(mine.n_union, off, 64), __shfl_down(mine.index, off, 64)};
        if (beats(o, mine)) mine = o;
    }
    if ((t & (kWave - 1)) == 0) sc[t / kWave] = mine;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int j = 1; j < kWaves; ++j)
            if (beats(sc[j], mine)) mine = sc[j];
        best[b] = mine.index;
        best_counts[3 * b] = s[2 * mine.index];
        best_counts[3 * b + 1] = s[2 * mine.index + 1];
        best_counts[3 * b + 2] = nm;
    }
}

int check_poses(const char* what, int P)
{
    return (P < 1 || P > kMaxPoses) ? rn_set_error(RN_E_INVALID, "%s: P=%d candidates (1..%d per call)", what, P, kMaxPoses) : RN_OK;
}

int check_image(const char* what, int ph, int pw)
{
    return (ph < 1 || pw < 1 || ph > kMaxSide || pw > kMaxSide)
               ? rn_set_error(RN_E_INVALID, "%s: a window of %d x %d pixels (1..%d each: the splat image lives in LDS)", what, ph, pw, kMaxSide)
               : RN_OK;
}

}  // namespace

extern "C" int rn_mask_pack(const unsigned char* mask, unsigned* mask_bits, int* n_mask, int B, int ph, int pw, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || check_image(what, ph, pw)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {mask, mask_bits, n_mask}) || rn_check_aligned(what, mask_bits, 4, "mask_bits") ||
        rn_check_aligned(what, n_mask, 4, "n_mask"))
        return RN_E_INVALID;
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, mask, mask_bits, n_mask, ph, pw);
    return rn_check_launch(what);
}

extern "C" size_t rn_pose_score_workspace_bytes(int B, int S)
{
    if ((S != 32 && S != 64 && S != 128) || B < 0 || B > kMaxBatch) return 0;
    return (((size_t)B * ((size_t)S * S * S / 32) + (size_t)B) * sizeof(int) + 15) & ~(size_t)15;   // the lists, then the counts
}

extern "C" int rn_pose_score(const unsigned* bits, const unsigned* mask_bits, const long long* cam, int* scores,
                             unsigned char* splats, int B, int P, int S, int N, int pixels_per_cell, int row0, int col0, int ph,
                             int pw, int footprint, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* what = __func__;
    if (rn_check_grid_side_pow2(what, S) || rn_check_frame(what, B, N, pixels_per_cell, row0, col0, ph, pw) ||
        check_image(what, ph, pw) || check_poses(what, P))
        return RN_E_INVALID;
    if (footprint < 1 || footprint > kMaxFootprint)
        return rn_set_error(RN_E_INVALID, "%s: footprint=%d (1..%d)", what, footprint, kMaxFootprint);
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {bits, mask_bits, cam, scores}) || rn_check_aligned(what, bits, 4, "bits") ||
        rn_check_aligned(what, mask_bits, 4, "mask_bits") || rn_check_aligned(what, cam, 8, "cam") ||
        rn_check_aligned(what, scores, 4, "scores"))
        return RN_E_INVALID;
    if (workspace && rn_check_ws(what, workspace, workspace_bytes, rn_pose_score_workspace_bytes(B, S))) return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)P, (unsigned)B);
    const int n_words = S * S * S / 32;
    if (workspace) {
        int* words = (int*)workspace;
        int* counts = words + (size_t)B * n_words;
        hipLaunchKernelGGL(pose_words_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, bits, words, counts, n_words);
        hipLaunchKernelGGL(pose_score_kernel<true>, grid, dim3(kBlock), 0, st, bits, mask_bits, (const i64*)cam, words, counts, scores,
                           splats, P, S, row0, col0, ph, pw, footprint);
    } else {
        hipLaunchKernelGGL(pose_score_kernel<false>, grid, dim3(kBlock), 0, st, bits, mask_bits, (const i64*)cam, nullptr, nullptr,
                           scores, splats, P, S, row0, col0, ph, pw, footprint);
    }
    return rn_check_launch(what);
}

extern "C" int rn_pose_best(const int* scores, const int* n_mask, int* best, int* best_counts, int B, int P, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || check_poses(what, P)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {scores, n_mask, best, best_counts}) || rn_check_aligned(what, scores, 4, "scores") ||
        rn_check_aligned(what, n_mask, 4, "n_mask") || rn_check_aligned(what, best, 4, "best") ||
        rn_check_aligned(what, best_counts, 4, "best_counts"))
        return RN_E_INVALID;
    hipLaunchKernelGGL(pose_best_kernel, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, scores, n_mask, best, best_counts, P);
    return rn_check_launch(what);
}
