// Voxel ray caster: the exact normal map of an occupancy grid at a pose, as 8-bit training targets (gfx950).
//
// The reference's ground truth came from an offline renderer (normal maps of each model at the pose named in the file
// name); for an occupancy grid it is computed here on the device: one orthographic ray per image pixel through the
// source grid, with the very M_inv the resampler uses (rn_pose_to_affine), first occupied voxel, integer normal, bytes.
// Geometry, traversal, normal rule and encoding are stated in include/rendernet_hip.h (rn_raycast_fwd); the float64 twin
// is tests/raycast_ref.py.  This file is built with -ffp-contract=off: kernel and twin read the same expressions.
//
//   rn_voxel_pack    float32 | uint8 voxels -> 1 bit per voxel (bit i of word i/32 = flat voxel index i) + per-item
//                    occupied bounding box.  One voxel per lane, one __ballot per wave = two words; the box is reduced
//                    per mask word (its first and last occupied lane), through LDS atomics per block, then at most
//                    six global atomics per block.
//   rn_raycast_fwd   one thread per pixel; a 256-thread block is a 16x16 pixel tile, each wave an 8x8 sub-tile, so the
//                    rays of a wave walk neighbouring voxels.  S <= 64: the item's occupied z-slab of the bit mask (at
//                    most 32 KB) is staged in LDS once per block; S = 128 (256 KB) reads the mask through the cache.
//                    The DDA recomputes each axis's next crossing from the integer boundary, t = (b - o) * (1 / dir),
//                    instead of accumulating increments: the coordinate error stays at a few float32 ulps of the grid
//                    size however long the ray is.
#include "rn_common.h"

namespace {

constexpr int kTile = 16;                 // pixel tile side of one 256-thread block
constexpr int kLdsWords = 64 * 64 * 64 / 32;

__global__ void box_init_kernel(int* __restrict__ box, int B, int S)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * 6) box[i] = (i % 6) < 3 ? S : -1;          // empty: lo = S, hi = -1
}

template <typename T>
__global__ __launch_bounds__(256)
void voxel_pack_kernel(const T* __restrict__ vox, float threshold, unsigned* __restrict__ bits, int* __restrict__ box,
                       int S, int words_per_item)
{
    __shared__ int sbox[6];
    const int b = blockIdx.y;
    const int per_item = words_per_item * 32;
    if (threadIdx.x < 6) sbox[threadIdx.x] = threadIdx.x < 3 ? S : -1;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;           // flat voxel index in the item; per_item % 256 == 0
    const bool on = (float)vox[(size_t)b * per_item + i] > threshold;
    const unsigned long long m = __ballot(on);
    const int lane = threadIdx.x & 63;
    if (lane == 0) bits[(size_t)b * words_per_item + (i >> 5)] = (unsigned)m;
    if (lane == 32) bits[(size_t)b * words_per_item + (i >> 5)] = (unsigned)(m >> 32);
    // the 32 lanes of a mask word lie in one x-row (S % 32 == 0): its lowest and highest occupied lanes carry the row's box
    const unsigned half = lane < 32 ? (unsigned)m : (unsigned)(m >> 32);
    if (on && ((lane & 31) == __ffs((int)half) - 1 || (lane & 31) == 31 - __clz((int)half))) {
        const int x = i % S, y = (i / S) % S, z = i / (S * S);
        atomicMin(&sbox[0], x); atomicMin(&sbox[1], y); atomicMin(&sbox[2], z);
        atomicMax(&sbox[3], x); atomicMax(&sbox[4], y); atomicMax(&sbox[5], z);
    }
    __syncthreads();
    if (threadIdx.x < 6 && sbox[5] >= 0) {
        if (threadIdx.x < 3) atomicMin(&box[b * 6 + threadIdx.x], sbox[threadIdx.x]);
        else atomicMax(&box[b * 6 + threadIdx.x], sbox[threadIdx.x]);
    }
}

// Occupancy of one item.  LDS form: words [w0, w0 + nw) of the item's mask (the occupied z-slab); everything the traversal
// and the normal stencil ask for outside it is outside the bounding box and therefore empty.
template <bool LDS>
struct Occ {
    const unsigned* words;     // LDS: the staged slab; otherwise the item's mask in global memory
    int S, w0, nw;

    __device__ __forceinline__ unsigned word(int w) const
    {
        if (LDS) {
            w -= w0;
            return ((unsigned)w < (unsigned)nw) ? words[w] : 0u;
        }
        return words[w];
    }
    // voxel (x, y, z); coordinates outside [0, S) are empty
    __device__ __forceinline__ bool at(int x, int y, int z) const
    {
        if ((unsigned)x >= (unsigned)S || (unsigned)y >= (unsigned)S || (unsigned)z >= (unsigned)S) return false;
        const int i = (z * S + y) * S + x;
        return (word(i >> 5) >> (i & 31)) & 1u;
    }
    // bits x0 .. x0+n-1 (n <= 7) of row (y, z) as the low n bits; outside the grid is empty
    __device__ __forceinline__ unsigned row(int x0, int n, int y, int z) const
    {
        if ((unsigned)y >= (unsigned)S || (unsigned)z >= (unsigned)S) return 0u;
        const int base = (z * S + y) * S;                   // multiple of 32
        unsigned long long v = 0;
        const int wx = x0 >> 5;                             // arithmetic shift: -1 for x0 in [-7, -1]
        const unsigned lo = (wx >= 0 && wx * 32 < S) ? word((base >> 5) + wx) : 0u;
        const unsigned hi = (wx + 1 >= 0 && (wx + 1) * 32 < S) ? word((base >> 5) + wx + 1) : 0u;
        v = ((unsigned long long)hi << 32) | lo;
        return (unsigned)(v >> (x0 - wx * 32)) & ((1u << n) - 1u);
    }
};

template <bool LDS>
__global__ __launch_bounds__(256)
void raycast_kernel(const unsigned* __restrict__ bits, const int* __restrict__ box, const float* __restrict__ m_inv,
                    unsigned char* __restrict__ out_u8, int* __restrict__ hit_id, signed char* __restrict__ face_out,
                    int S, int N, int f, int row0, int col0, int ph, int pw, int R, int low_x)
{
    __shared__ unsigned slab[LDS ? kLdsWords : 1];
    const int b = blockIdx.z;
    const int words_per_item = S * S * (S / 32);
    const unsigned* item = bits + (size_t)b * words_per_item;
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {                           // clamped: a box from elsewhere must not index past the mask
        lo[k] = max(box[b * 6 + k], 0);
        hi[k] = min(box[b * 6 + 3 + k], S - 1);
    }
    const bool empty = hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2];      // block-uniform

    Occ<LDS> occ;
    occ.S = S;
    if (LDS) {
        const int wz = S * (S / 32);                        // words per z-layer
        occ.w0 = empty ? 0 : lo[2] * wz;
        occ.nw = empty ? 0 : (hi[2] - lo[2] + 1) * wz;      // multiple of 32 words: uint4 copies
        const uint4* src = reinterpret_cast<const uint4*>(item + occ.w0);
        uint4* dst = reinterpret_cast<uint4*>(slab);
        for (int i = threadIdx.x; i < occ.nw / 4; i += 256) dst[i] = src[i];
        occ.words = slab;
        __syncthreads();
    } else {
        occ.w0 = 0;
        occ.nw = words_per_item;
        occ.words = item;
    }

    // 16x16 tile = 2x2 waves of 8x8 pixels
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pr = blockIdx.y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const int pc = blockIdx.x * kTile + (wave & 1) * 8 + (lane & 7);
    if (pr >= ph || pc >= pw) return;
    const size_t px = ((size_t)b * ph + pr) * pw + pc;

    int hit = -1, face = 0;
    unsigned char rgb[3] = {0, 0, 0};
    if (!empty) {
        const float* M = m_inv + (size_t)b * 12;
        const float fN = (float)N;
        const float y = (float)(N - 1) - (((float)(row0 + pr) + 0.5f) / (float)f - 0.5f);
        const float z = ((float)(col0 + pc) + 0.5f) / (float)f - 0.5f;
        const float x0 = low_x ? -0.5f : fN - 0.5f;
        float o[3], dir[3], inv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = ((M[4 * k] * x0 + M[4 * k + 1] * y) + M[4 * k + 2] * z) + M[4 * k + 3];
            dir[k] = low_x ? M[4 * k] : -M[4 * k];
            inv[k] = 1.0f / dir[k];                         // +-inf for an axis the ray never crosses; not used then
        }
        // clip against the occupied box [lo - 0.5, hi + 0.5]^3
        float tenter = 0.0f, texit = fN, t0max = -INFINITY;
        int eaxis = 0;
        bool alive = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float blo = (float)lo[k] - 0.5f, bhi = (float)hi[k] + 0.5f;
            if (dir[k] != 0.0f) {
                const float ta = (blo - o[k]) * inv[k], tb = (bhi - o[k]) * inv[k];
                const float t0 = dir[k] > 0.0f ? ta : tb, t1 = dir[k] > 0.0f ? tb : ta;
                if (t0 > t0max) { t0max = t0; eaxis = k; }
                texit = fminf(texit, t1);
            } else if (!(o[k] >= blo && o[k] < bhi)) {
                alive = false;
            }
        }
        tenter = fmaxf(tenter, t0max);
        alive = alive && tenter < texit;
        if (alive) {
            int v[3], sgn[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sgn[k] = dir[k] > 0.0f ? 1 : -1;
                const int q = (int)floorf((o[k] + tenter * dir[k]) + 0.5f);
                v[k] = min(max(q, lo[k]), hi[k]);
            }
            if (t0max > 0.0f) v[eaxis] = dir[eaxis] > 0.0f ? lo[eaxis] : hi[eaxis];
            face = 2 * eaxis + (dir[eaxis] < 0.0f ? 1 : 0);
            for (int step = 0; step < 3 * S + 3; ++step) {
                if (occ.at(v[0], v[1], v[2])) { hit = (v[2] * S + v[1]) * S + v[0]; break; }
                float tmin = INFINITY;
                int a = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float t = dir[k] != 0.0f ? (((float)v[k] + 0.5f * (float)sgn[k]) - o[k]) * inv[k] : INFINITY;
                    if (t < tmin) { tmin = t; a = k; }
                }
                if (!(tmin <= fN)) break;                   // the ray ends at t = N
                if (a == 0) v[0] += sgn[0]; else if (a == 1) v[1] += sgn[1]; else v[2] += sgn[2];
                const int va = a == 0 ? v[0] : a == 1 ? v[1] : v[2];
                const int la = a == 0 ? lo[0] : a == 1 ? lo[1] : lo[2], ha = a == 0 ? hi[0] : a == 1 ? hi[1] : hi[2];
                if (va < la || va > ha) break;              // left the occupied box
                const float da = a == 0 ? dir[0] : a == 1 ? dir[1] : dir[2];
                face = 2 * a + (da < 0.0f ? 1 : 0);
            }
        }
        if (hit >= 0) {
            const int vx = hit % S, vy = (hit / S) % S, vz = hit / (S * S);
            int g[3] = {0, 0, 0};
            const int n = 2 * R + 1;
            for (int dz = -R; dz <= R; ++dz) {
                for (int dy = -R; dy <= R; ++dy) {
                    const unsigned w = occ.row(vx - R, n, vy + dy, vz + dz);
                    const int cnt = __popc(w);
                    int sx = 0;
                    for (int i = 0; i < n; ++i) sx += ((w >> i) & 1u) ? i - R : 0;
                    g[0] += sx; g[1] += dy * cnt; g[2] += dz * cnt;
                }
            }
            const int ea = face >> 1, es = (face & 1) ? 1 : -1;
            int ns[3] = {-g[0], -g[1], -g[2]};
            const int ne = (ea == 0 ? ns[0] : ea == 1 ? ns[1] : ns[2]) * es;
            if (ne <= 0) {                                  // covers g == 0
                ns[0] = ea == 0 ? es : 0; ns[1] = ea == 1 ? es : 0; ns[2] = ea == 2 ? es : 0;
            }
            // camera-grid normal n = M_lin^T n_src
            float c[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                c[j] = (M[j] * (float)ns[0] + M[4 + j] * (float)ns[1]) + M[8 + j] * (float)ns[2];
            const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
            const float comp[3] = {c[2] / len, c[1] / len, (low_x ? -c[0] : c[0]) / len};   // right, up, towards
#pragma unroll
            for (int j = 0; j < 3; ++j) rgb[j] = (unsigned char)(int)rintf(255.0f * (0.5f + 0.5f * comp[j]));
        }
    }
    out_u8[px * 3 + 0] = rgb[0];
    out_u8[px * 3 + 1] = rgb[1];
    out_u8[px * 3 + 2] = rgb[2];
    if (hit_id) hit_id[px] = hit;
    if (face_out) face_out[px] = (signed char)(hit >= 0 ? face : 0);
}

}  // namespace

extern "C" int rn_voxel_pack(const void* vox, int vox_is_u8, float threshold, unsigned* bits, int* box, int B, int S,
                             void* stream)
{
    if (B < 0) return rn_set_error(RN_E_INVALID, "rn_voxel_pack: B=%d", B);
    if (S < 32 || S > 128 || S % 32 != 0)
        return rn_set_error(RN_E_INVALID, "rn_voxel_pack: S=%d (a multiple of 32 up to 128)", S);
    if (vox_is_u8 != 0 && vox_is_u8 != 1) return rn_set_error(RN_E_INVALID, "rn_voxel_pack: vox_is_u8=%d", vox_is_u8);
    if (!(threshold == threshold)) return rn_set_error(RN_E_INVALID, "rn_voxel_pack: threshold is NaN");
    if (B == 0) return RN_OK;
    if (B > 65535) return rn_set_error(RN_E_INVALID, "rn_voxel_pack: B=%d (at most 65535 per call)", B);
    if (!vox || !bits || !box) return rn_set_error(RN_E_INVALID, "rn_voxel_pack: null pointer");
    if (((uintptr_t)bits & 15) != 0 || ((uintptr_t)box & 3) != 0 || (!vox_is_u8 && ((uintptr_t)vox & 3) != 0))
        return rn_set_error(RN_E_INVALID, "rn_voxel_pack: bits must be 16-byte aligned, box and float voxels 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int words = S * S * (S / 32);
    hipLaunchKernelGGL(box_init_kernel, dim3((unsigned)((B * 6 + 255) / 256)), dim3(256), 0, st, box, B, S);
    const dim3 grid((unsigned)(words * 32 / 256), (unsigned)B);
    if (vox_is_u8)
        hipLaunchKernelGGL(voxel_pack_kernel<unsigned char>, grid, dim3(256), 0, st, (const unsigned char*)vox, threshold,
                           bits, box, S, words);
    else
        hipLaunchKernelGGL(voxel_pack_kernel<float>, grid, dim3(256), 0, st, (const float*)vox, threshold, bits, box, S,
                           words);
    return rn_check_launch("rn_voxel_pack");
}

extern "C" int rn_raycast_fwd(const unsigned* bits, const int* box, const float* m_inv, unsigned char* out_u8, int* hit_id,
                              signed char* face, int B, int S, int N, int pixels_per_cell, int row0, int col0, int ph,
                              int pw, int normal_radius, int view_from_low_x, void* stream)
{
    const int f = pixels_per_cell;
    if (B < 0) return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: B=%d", B);
    if (S < 32 || S > 128 || S % 32 != 0)
        return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: S=%d (a multiple of 32 up to 128)", S);
    if (N < 1 || N > 256) return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: N=%d (1..256)", N);
    if (f < 1 || f > 16) return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: pixels_per_cell=%d (1..16)", f);
    if (normal_radius < 1 || normal_radius > 3)
        return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: normal_radius=%d (1..3)", normal_radius);
    if (view_from_low_x != 0 && view_from_low_x != 1)
        return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: view_from_low_x=%d", view_from_low_x);
    const int F = f * N;
    if (row0 < 0 || col0 < 0 || ph < 1 || pw < 1 || ph > F - row0 || pw > F - col0)
        return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: window rows %d+%d cols %d+%d outside the %dx%d frame", row0, ph,
                            col0, pw, F, F);
    if (B == 0) return RN_OK;
    if (B > 65535) return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: B=%d (at most 65535 per call)", B);
    if (!bits || !box || !m_inv || !out_u8) return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: null pointer");
    if (((uintptr_t)bits & 15) != 0 || ((uintptr_t)box & 3) != 0 || ((uintptr_t)m_inv & 3) != 0 || ((uintptr_t)hit_id & 3) != 0)
        return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: bits must be 16-byte aligned, box, m_inv and hit_id 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((pw + kTile - 1) / kTile), (unsigned)((ph + kTile - 1) / kTile), (unsigned)B);
    if (S <= 64)
        hipLaunchKernelGGL(raycast_kernel<true>, grid, dim3(256), 0, st, bits, box, m_inv, out_u8, hit_id, face, S, N, f,
                           row0, col0, ph, pw, normal_radius, view_from_low_x);
    else
        hipLaunchKernelGGL(raycast_kernel<false>, grid, dim3(256), 0, st, bits, box, m_inv, out_u8, hit_id, face, S, N, f,
                           row0, col0, ph, pw, normal_radius, view_from_low_x);
    return rn_check_launch("rn_raycast_fwd");
}
