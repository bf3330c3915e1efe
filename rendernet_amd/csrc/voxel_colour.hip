// Voxel colouring: the colour of posed pictures taken back onto the grid they show, the inverse of the albedo caster (gfx950).
// The rule -- which pixels count, the sums, the rounded means, the Jacobi fill, the cell of a vertex, the limits and the bounds
// -- is stated in include/rendernet_hip.h (rn_voxel_colour_accumulate and its neighbours); the NumPy twin is
// tests/voxel_colour_ref.py.  Everything is integer: no float appears in this file.
//
//   colour_accumulate_kernel  the hot path, a scatter.  lane = pixel, blockIdx.y = item, blockIdx.x walks the K ph pw pixels of
//                       the item's views in memory order; a wave takes kChunks chunks of 64 neighbouring pixels of ONE item -- a
//                       chunk may span two views, whose destinations are the same grid, never two grids.  A voxel covers a few
//                       pixels of a row, so neighbouring lanes mostly share a destination: the heads of the runs of equal hit
//                       ids are found with one shuffle and one ballot, every lane gets the number of its run, and a shuffle-down
//                       tree (1, 2, .. 32) that joins only lanes of the same run number leaves each run's sum in its head.  A
//                       pixel that does not count has run number -1 - lane, so it joins nothing and breaks the run it stands in.
//                       A chunk's partial sums stay below 64 * 255 < 2^16: red | green << 16 and blue | count << 16 travel as
//                       two words.  The atomics are counted in 64-byte requests at the memory side, so the four words of a run
//                       must not go out as four instructions: the heads are compacted to the low lanes (one push permute, the
//                       slots being a permutation of the lanes) and read back sixteen at a time, four neighbouring lanes adding
//                       the four neighbouring words of one run.  Integer adds commute: the sums do not depend on the order of
//                       arrival.  DESIGN.md 5c has the timing of this form and of the head-adds-four-words form before it.
//   colour_resolve_kernel, colour_fill_kernel, colour_from_hits_kernel, vertex_colours_kernel
//                       plain gathers, one thread per voxel, pixel or vertex; every index is bounds-tested before it is used.
#include "voxel_common.h"
#include "raycast_common.h"

namespace {

constexpr long long kMaxPixelsPerItem = 8421504;      // K ph pw of one call: 255 times it is 2 147 483 520 < 2^31
static_assert(kMaxPixelsPerItem * 255 < (1ll << 31) && (kMaxPixelsPerItem + 1) * 255 >= (1ll << 31), "the largest K ph pw that cannot wrap");
constexpr int kMaxViews = 65535;

__device__ __forceinline__ int rounded_mean(long long sigma, long long n)      // n > 0; a byte whatever sigma holds
{
    const long long v = (2 * sigma + n) / (2 * n);
    return (int)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

constexpr int kChunks = 4;                 // 64-pixel chunks a wave walks one after the other
constexpr int kWavePixels = kWave * kChunks, kBlockPixels = kBlock * kChunks;

__global__ __launch_bounds__(kBlock)
void colour_accumulate_kernel(const unsigned char* __restrict__ images, const int* __restrict__ hits,
                              const unsigned char* __restrict__ mask, int* __restrict__ sums, int item_px, int cells)
{
    const int b = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1);
    const int first = (int)blockIdx.x * kBlockPixels + (int)(threadIdx.x / kWave) * kWavePixels + lane;   // < 8421504 + 1024
    const size_t item = (size_t)b * item_px;
    int hit[kChunks];
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {                                   // all the loads of the wave's pixels are in flight at once
        const int p = first + j * kWave;
        hit[j] = p < item_px ? hits[item + p] : -1;
    }
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
        // no lane leaves the loop and every branch around a shuffle is wave-uniform: all 64 lanes take part in each of them
        const size_t px = item + first + j * kWave;
        int key = -1;                                                     // the hit id of a pixel that counts
        unsigned rg = 0, bn = 0;
        if ((unsigned)hit[j] < (unsigned)cells && (mask == nullptr || mask[px] != 0)) {      // a hit in range lies inside the item
            key = hit[j];
            const unsigned char* c = images + px * 3;
            rg = (unsigned)c[0] | (unsigned)c[1] << 16;
            bn = (unsigned)c[2] | 1u << 16;
        }
        const int before = __shfl_up(key, 1, kWave);
        const bool head = key >= 0 && (lane == 0 || before != key);
        const unsigned long long heads = __ballot(head);
        if (heads == 0) continue;                                         // wave-uniform: nothing in this chunk counts
        const int heads_below = lanes_before(heads);
        // heads at or before this lane: 1.. for a pixel that counts, the same number exactly for the lanes of one run
        const int run = key >= 0 ? heads_below + (head ? 1 : 0) : -1 - lane;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int r2 = __shfl_down(run, d, kWave);
            const unsigned rg2 = __shfl_down(rg, d, kWave), bn2 = __shfl_down(bn, d, kWave);
            if (lane + d < kWave && r2 == run) {
                rg += rg2;
                bn += bn2;
            }
        }
        // the heads move to lanes 0 .. n_heads - 1 in their order and the other lanes behind them: `slot` is a permutation of
        // the 64 lanes, so every lane of the push receives exactly one value
        const int n_heads = __popcll(heads);
        const int slot = head ? heads_below : n_heads + (lane - heads_below);
        const int key_c = __builtin_amdgcn_ds_permute(slot * 4, key);
        const unsigned rg_c = (unsigned)__builtin_amdgcn_ds_permute(slot * 4, (int)rg);
        const unsigned bn_c = (unsigned)__builtin_amdgcn_ds_permute(slot * 4, (int)bn);
        // sixteen runs per instruction: four neighbouring lanes add the four neighbouring words of one run
        for (int i = 0; i < n_heads; i += kWave / 4) {                    // n_heads is wave-uniform
            const int src = i + (lane >> 2);                              // <= 48 + 15
            const int k = __shfl(key_c, src, kWave);
            const unsigned a = __shfl(rg_c, src, kWave), c = __shfl(bn_c, src, kWave);
            if (src < n_heads) {                                          // lane src holds a head: 0 <= k < cells
                const unsigned w = (lane & 2) ? c : a;
                int* dst = sums + ((size_t)b * cells + (size_t)k) * 4;    // 64 bits, and only after the range test
                atomicAdd(dst + (lane & 3), (int)((lane & 1) ? w >> 16 : w & 0xffffu));
            }
        }
    }
}

__global__ __launch_bounds__(kBlock)
void colour_resolve_kernel(const int4* __restrict__ sums, unsigned char* __restrict__ colour, unsigned char* __restrict__ known,
                           size_t total, int ur, int ug, int ub)
{
    const size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= total) return;
    const int4 s = sums[v];
    int r = ur, g = ug, bl = ub;
    if (s.w > 0) {
        r = rounded_mean(s.x, s.w);
        g = rounded_mean(s.y, s.w);
        bl = rounded_mean(s.z, s.w);
    }
    colour[v * 3] = (unsigned char)r;
    colour[v * 3 + 1] = (unsigned char)g;
    colour[v * 3 + 2] = (unsigned char)bl;
    known[v] = s.w > 0 ? 1 : 0;
}

// one Jacobi pass: thread = voxel, blockIdx.y = item; reads the state before the pass only
__global__ __launch_bounds__(kBlock)
void colour_fill_kernel(const unsigned char* __restrict__ colour_in, const unsigned char* __restrict__ known_in,
                        const unsigned* __restrict__ bits, unsigned char* __restrict__ colour_out,
                        unsigned char* __restrict__ known_out, int S)
{
    const int cells = S * S * S;
    const int v = (int)blockIdx.x * kBlock + (int)threadIdx.x;            // S^3 is a multiple of 256
    const size_t item = (size_t)blockIdx.y * cells;
    const unsigned char* __restrict__ kin = known_in + item;
    const unsigned char* __restrict__ cin = colour_in + item * 3;
    int kn = kin[v], r = cin[(size_t)v * 3], g = cin[(size_t)v * 3 + 1], bl = cin[(size_t)v * 3 + 2];
    const bool occupied = (bits[(item + v) >> 5] >> (v & 31)) & 1u;
    if (kn == 0 && occupied) {
        const int x = v % S, y = (v / S) % S, z = v / (S * S);
        int sr = 0, sg = 0, sb = 0, m = 0;                                // at most 26 * 255
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int zz = z + dz, yy = y + dy, xx = x + dx;
                    if ((dz | dy | dx) == 0 || (unsigned)zz >= (unsigned)S || (unsigned)yy >= (unsigned)S || (unsigned)xx >= (unsigned)S)
                        continue;
                    const int u = (zz * S + yy) * S + xx;
                    if (kin[u] != 0) {
                        sr += cin[(size_t)u * 3];
                        sg += cin[(size_t)u * 3 + 1];
                        sb += cin[(size_t)u * 3 + 2];
                        ++m;
                    }
                }
        if (m > 0) {
            r = rounded_mean(sr, m);
            g = rounded_mean(sg, m);
            bl = rounded_mean(sb, m);
            kn = 2;
        }
    }
    unsigned char* co = colour_out + (item + v) * 3;
    co[0] = (unsigned char)r;
    co[1] = (unsigned char)g;
    co[2] = (unsigned char)bl;
    known_out[item + v] = (unsigned char)kn;
}

__global__ __launch_bounds__(kBlock)
void colour_from_hits_kernel(const int* __restrict__ hit_id, const unsigned char* __restrict__ colour, unsigned char* __restrict__ out,
                             int item_px, int cells, int br, int bg, int bb)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= item_px) return;
    const size_t px = (size_t)blockIdx.y * item_px + p;
    const int hit = hit_id[px];
    int r = br, g = bg, bl = bb;
    if ((unsigned)hit < (unsigned)cells) {
        const unsigned char* c = colour + ((size_t)blockIdx.y * cells + (size_t)hit) * 3;
        r = c[0];
        g = c[1];
        bl = c[2];
    }
    out[px * 3] = (unsigned char)r;
    out[px * 3 + 1] = (unsigned char)g;
    out[px * 3 + 2] = (unsigned char)bl;
}

// thread = vertex; its grid is the last b with vert_offsets[b] <= v, searched inside 0 .. B-1 whatever the offsets hold
__global__ __launch_bounds__(kBlock)
void vertex_colours_kernel(const int* __restrict__ verts, long long V, const long long* __restrict__ vert_offsets,
                           const unsigned char* __restrict__ colour, const unsigned char* __restrict__ known,
                           unsigned char* __restrict__ out, int B, int S, int ur, int ug, int ub)
{
    const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (vert_offsets[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    const size_t item = (size_t)lo * S * S * S;
    long long cell[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) cell[j] = ((long long)verts[v * 3 + j] + 128) >> 8;          // arithmetic shift: floor
    int sr = 0, sg = 0, sb = 0, m = 0;
    for (int c = 0; c < 8; ++c) {
        const long long z = cell[0] - 1 + (c >> 2), y = cell[1] - 1 + ((c >> 1) & 1), x = cell[2] - 1 + (c & 1);
        if (z < 0 || z >= S || y < 0 || y >= S || x < 0 || x >= S) continue;
        const size_t u = item + (size_t)((z * S + y) * S + x);
        if (known[u] != 0) {
            sr += colour[u * 3];
            sg += colour[u * 3 + 1];
            sb += colour[u * 3 + 2];
            ++m;
        }
    }
    out[v * 3] = (unsigned char)(m ? rounded_mean(sr, m) : ur);
    out[v * 3 + 1] = (unsigned char)(m ? rounded_mean(sg, m) : ug);
    out[v * 3 + 2] = (unsigned char)(m ? rounded_mean(sb, m) : ub);
}

int check_colour(const char* what, const char* name, int r, int g, int b)
{
    return (r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255)
               ? rn_set_error(RN_E_INVALID, "%s: %s (%d, %d, %d), each 0..255", what, name, r, g, b) : RN_OK;
}

int check_views(const char* what, int K, int ph, int pw)
{
    if (K < 1 || K > kMaxViews) return rn_set_error(RN_E_INVALID, "%s: K=%d views (1..%d)", what, K, kMaxViews);
    if (rn_check_window(what, ph, pw)) return RN_E_INVALID;
    if ((long long)K * ph * pw > kMaxPixelsPerItem)
        return rn_set_error(RN_E_INVALID, "%s: K ph pw = %lld pixels per item (at most %lld per call: 255 times more would wrap an int32 sum)",
                            what, (long long)K * ph * pw, kMaxPixelsPerItem);
    return RN_OK;
}

}  // namespace

extern "C" int rn_voxel_colour_accumulate(const unsigned char* images, const int* hits, const unsigned char* mask, int* sums, int B,
                                          int K, int S, int ph, int pw, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || rn_check_grid_side_pow2(what, S) || check_views(what, K, ph, pw)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {images, hits, sums}) || rn_check_aligned(what, hits, 4, "hits") || rn_check_aligned(what, sums, 16, "sums"))
        return RN_E_INVALID;
    const int item_px = K * ph * pw;
    hipLaunchKernelGGL(colour_accumulate_kernel, dim3((unsigned)((item_px + kBlockPixels - 1) / kBlockPixels), (unsigned)B), dim3(kBlock),
                       0, (hipStream_t)stream, images, hits, mask, sums, item_px, S * S * S);
    return rn_check_launch(what);
}

extern "C" int rn_voxel_colour_resolve(const int* sums, unsigned char* colour, unsigned char* known, int B, int S, int unseen_r,
                                       int unseen_g, int unseen_b, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || rn_check_grid_side_pow2(what, S) || check_colour(what, "unseen", unseen_r, unseen_g, unseen_b))
        return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {sums, colour, known}) || rn_check_aligned(what, sums, 16, "sums")) return RN_E_INVALID;
    const size_t total = (size_t)B * S * S * S;                           // a multiple of 256, at most 65535 * 2^21
    hipLaunchKernelGGL(colour_resolve_kernel, dim3((unsigned)(total / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const int4*)sums, colour, known, total, unseen_r, unseen_g, unseen_b);
    return rn_check_launch(what);
}

extern "C" int rn_voxel_colour_fill(const unsigned char* colour_in, const unsigned char* known_in, const unsigned* bits,
                                    unsigned char* colour_out, unsigned char* known_out, int B, int S, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || rn_check_grid_side_pow2(what, S)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {colour_in, known_in, bits, colour_out, known_out}) || rn_check_aligned(what, bits, 4, "bits"))
        return RN_E_INVALID;
    if (colour_in == colour_out || known_in == known_out)
        return rn_set_error(RN_E_INVALID, "%s: a pass reads the state before it: the output buffers must be other ones", what);
    hipLaunchKernelGGL(colour_fill_kernel, dim3((unsigned)(S * S * S / kBlock), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream,
                       colour_in, known_in, bits, colour_out, known_out, S);
    return rn_check_launch(what);
}

extern "C" int rn_colour_from_hits(const int* hit_id, const unsigned char* colour, unsigned char* out_u8, int B, int S, int ph, int pw,
                                   int background_r, int background_g, int background_b, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || rn_check_grid_side_pow2(what, S) || rn_check_window(what, ph, pw) ||
        check_colour(what, "background", background_r, background_g, background_b))
        return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_pointers(what, {hit_id, colour, out_u8}) || rn_check_aligned(what, hit_id, 4, "hit_id")) return RN_E_INVALID;
    const int item_px = ph * pw;                                          // at most 2^24
    hipLaunchKernelGGL(colour_from_hits_kernel, dim3((unsigned)((item_px + kBlock - 1) / kBlock), (unsigned)B), dim3(kBlock), 0,
                       (hipStream_t)stream, hit_id, colour, out_u8, item_px, S * S * S, background_r, background_g, background_b);
    return rn_check_launch(what);
}

extern "C" int rn_mesh_vertex_colours(const int* verts, long long V, const long long* vert_offsets, const unsigned char* colour,
                                      const unsigned char* known, unsigned char* out_u8, int B, int S, int unseen_r, int unseen_g,
                                      int unseen_b, void* stream)
{
    const char* what = __func__;
    if (rn_check_batch(what, B) || rn_check_grid_side_pow2(what, S) || check_colour(what, "unseen", unseen_r, unseen_g, unseen_b))
        return RN_E_INVALID;
    if (V < 0 || V > (1ll << 31) - 1) return rn_set_error(RN_E_INVALID, "%s: V=%lld vertices (0..2^31 - 1)", what, V);
    if (B == 0 && V != 0) return rn_set_error(RN_E_INVALID, "%s: %lld vertices of no grid", what, V);
    if (B == 0 || V == 0) return RN_OK;
    if (rn_check_pointers(what, {verts, vert_offsets, colour, known, out_u8}) || rn_check_aligned(what, verts, 4, "verts") ||
        rn_check_aligned(what, vert_offsets, 8, "vert_offsets"))
        return RN_E_INVALID;
    hipLaunchKernelGGL(vertex_colours_kernel, dim3((unsigned)((V + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, verts,
                       V, vert_offsets, colour, known, out_u8, B, S, unseen_r, unseen_g, unseen_b);
    return rn_check_launch(what);
}
