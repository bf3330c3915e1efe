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
//   rn_raycast_ao_fwd  ambient occlusion of the hit faces: 64 rays per (hit voxel, entry face), one per lane of a wave, walked
//                    with the same DDA through the same slab; the count of open rays is one ballot (raycast_ao_kernel).
//   rn_ao_encode     counts -> bytes, a masked integer mean over a pixel window (ao_encode_kernel).
//   rn_raycast_edges_fwd  silhouette, depth and crease bits of every hit pixel against the hits within line_radius pixels:
//                    the tile and its halo are staged in LDS as (packed hit voxel, integer normal), then compared pairwise
//                    (raycast_edges_kernel).  Integers only.
//   rn_lines_encode  normal bytes + edge bits -> ink, white, or a diffuse band under a quantised light (lines_encode_kernel).
//   rn_shadow_light  the light per item as an integer direction in source-grid coordinates (shadow_light_kernel).
//   rn_raycast_shadow_fwd  hard cast shadows of the hit faces: one integer DDA per pixel from the centre of the entry face
//                    towards the light, through the same slab (raycast_shadow_kernel).  Integers only.
//   rn_shadow_encode normal bytes + lit flags -> ambient + diffuse * the masked mean of lit over a pixel window
//                    (shadow_encode_kernel).
// The window mean of the two encode kernels and the argument checks the entry points have in common are in raycast_common.h,
// shared with raycast_albedo.hip.
#include "raycast_common.h"
#include "ao_dirs.h"

namespace {

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

// The occupancy of one item for a whole block: its box clamped to the grid (a box from elsewhere must not index past the
// mask) and, in the LDS form, its occupied z-slab staged in `slab` (every thread of the block calls this; it ends in a
// barrier).  Returns whether the item is empty (block-uniform).
template <bool LDS>
__device__ __forceinline__ bool open_item(const unsigned* __restrict__ item, const int* __restrict__ box6, int S,
                                          unsigned* slab, int lo[3], int hi[3], Occ<LDS>& occ)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = max(box6[k], 0);
        hi[k] = min(box6[3 + k], S - 1);
    }
    const bool empty = hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2];
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
        occ.nw = S * S * (S / 32);
        occ.words = item;
    }
    return empty;
}

// n_src of rn_raycast_fwd's rule for the hit voxel (vx, vy, vz) entered by `face`, in integers: -g over the {-R..R}^3
// stencil, or the entry face's outward unit vector when g == 0 or (-g).e <= 0.  |ns[k]| <= 6 * 49 = 294 for R = 3.
template <bool LDS>
__device__ __forceinline__ void source_normal(const Occ<LDS>& occ, int vx, int vy, int vz, int face, int R, int ns[3])
{
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
    ns[0] = -g[0]; ns[1] = -g[1]; ns[2] = -g[2];
    const int ne = (ea == 0 ? ns[0] : ea == 1 ? ns[1] : ns[2]) * es;
    if (ne <= 0) {                                          // covers g == 0
        ns[0] = ea == 0 ? es : 0; ns[1] = ea == 1 ? es : 0; ns[2] = ea == 2 ? es : 0;
    }
}

template <bool LDS>
__global__ __launch_bounds__(256)
void raycast_kernel(const unsigned* __restrict__ bits, const int* __restrict__ box, const float* __restrict__ m_inv,
                    unsigned char* __restrict__ out_u8, int* __restrict__ hit_id, signed char* __restrict__ face_out,
                    int S, int N, int f, int row0, int col0, int ph, int pw, int R, int low_x)
{
    __shared__ unsigned slab[LDS ? kLdsWords : 1];
    const int b = blockIdx.z;
    int lo[3], hi[3];
    Occ<LDS> occ;
    const bool empty = open_item<LDS>(bits + (size_t)b * (S * S * (S / 32)), box + b * 6, S, slab, lo, hi, occ);

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
            int ns[3];
            source_normal<LDS>(occ, hit % S, (hit / S) % S, hit / (S * S), face, R, ns);
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

// Ambient occlusion of the hit faces (include/rendernet_hip.h, rn_raycast_ao_fwd): same tile mapping and slab as
// raycast_kernel, but LANE = RAY.  A wave's 8x8 pixels see a handful of distinct (hit voxel, entry face) pairs; the wave takes
// the first pending lane's pair, all 64 lanes walk their own direction from that face, the open rays are counted with one
// ballot, and every lane whose own pair is the leader's takes the count.  No lane leaves before the loop: lanes outside the
// window, and misses, stay in the collectives with nothing pending.
template <bool LDS>
__global__ __launch_bounds__(256)
void raycast_ao_kernel(const unsigned* __restrict__ bits, const int* __restrict__ box, const int* __restrict__ hit_id,
                       const signed char* __restrict__ face_in, unsigned char* __restrict__ count, int S, int ph, int pw,
                       int L)
{
    __shared__ unsigned slab[LDS ? kLdsWords : 1];
    const int b = blockIdx.z;
    int lo[3], hi[3];
    Occ<LDS> occ;
    open_item<LDS>(bits + (size_t)b * (S * S * (S / 32)), box + b * 6, S, slab, lo, hi, occ);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pr = blockIdx.y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const int pc = blockIdx.x * kTile + (wave & 1) * 8 + (lane & 7);
    const bool inside = pr < ph && pc < pw;
    const size_t px = ((size_t)b * ph + pr) * pw + pc;

    int key = -1;                                           // hit * 8 + face; -1: nothing pending
    if (inside) {
        const int h = hit_id[px], fc = face_in[px];
        if (h >= 0 && h < S * S * S && fc >= 0 && fc < 6) key = h * 8 + fc;
    }
    const float tx = rn_ao_dirs[lane][0], ty = rn_ao_dirs[lane][1], tz = rn_ao_dirs[lane][2];
    int result = 255;

    unsigned long long pending = __ballot(key >= 0);
    while (pending != 0ull) {
        const int leader = __shfl(key, __ffsll(pending) - 1);
        const int h = leader >> 3, a = (leader >> 1) & 3, s = (leader & 1) ? 1 : -1;
        const int v[3] = {h % S, (h / S) % S, h / (S * S)};
        const float ds = (float)s * tx;
        const float d[3] = {a == 0 ? ds : a == 1 ? tz : ty, a == 0 ? ty : a == 1 ? ds : tz, a == 0 ? tz : a == 1 ? ty : ds};
        float inv[3], off[3];                               // off: the origin c relative to v, exact
        int sg[3], w[3];                                    // w: the visited voxel relative to v
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            inv[k] = 1.0f / d[k];                           // +-inf for an axis the ray never crosses; not used then
            sg[k] = d[k] > 0.0f ? 1 : -1;
            off[k] = k == a ? 0.5f * (float)s : 0.0f;
            w[k] = k == a ? s : 0;
        }
        bool open = true;
        for (int step = 0; step < 3 * L + 3; ++step) {
            const int u[3] = {v[0] + w[0], v[1] + w[1], v[2] + w[2]};
            if (u[0] < lo[0] || u[0] > hi[0] || u[1] < lo[1] || u[1] > hi[1] || u[2] < lo[2] || u[2] > hi[2]) break;   // left the box
            if (occ.at(u[0], u[1], u[2])) { open = false; break; }
            if (max(max(abs(w[0]), abs(w[1])), abs(w[2])) > L) break;
            float tmin = INFINITY;
            int m = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float t = d[k] != 0.0f ? (((float)w[k] + 0.5f * (float)sg[k]) - off[k]) * inv[k] : INFINITY;
                if (t < tmin) { tmin = t; m = k; }
            }
            if (m == 0) w[0] += sg[0]; else if (m == 1) w[1] += sg[1]; else w[2] += sg[2];
        }
        const int n_open = __popcll(__ballot(open));
        if (key == leader) { result = n_open; key = -1; }
        pending = __ballot(key >= 0);
    }
    if (inside) count[px] = (unsigned char)result;
}

// The bytes of the open-ray counts: a masked mean over the (2r+1)^2 window clipped to the frame, in integers (window_sum).
// A cell is (count | 1 << 16) per hit pixel, 0 per miss, so one sum carries both the counts and the number of hits (at most
// 289 * 64 < 2^16).
__global__ __launch_bounds__(256)
void ao_encode_kernel(const unsigned char* __restrict__ count, unsigned char* __restrict__ out, int ph, int pw, int r)
{
    __shared__ WindowCells<int> cell;
    __shared__ WindowRowSums<int> rowsum;
    const int b = blockIdx.z;
    const unsigned char* src = count + (size_t)b * ph * pw;
    const auto load = [=](int gr, int gc) {
        const int cval = src[(size_t)gr * pw + gc];
        return cval <= RN_AO_RAYS ? (cval | (1 << 16)) : 0;
    };
    int sum, centre;
    if (!window_sum<HaloLoad::clamped>(cell, rowsum, ph, pw, r, load, sum, centre)) return;   // after both barriers
    const int pr = blockIdx.y * kTile + threadIdx.x / kTile, pc = blockIdx.x * kTile + threadIdx.x % kTile;
    const int total = sum & 0xffff, n = sum >> 16;
    const bool is_hit = centre != 0;                        // then n >= 1
    out[((size_t)b * ph + pr) * pw + pc] = is_hit ? (unsigned char)((510 * total + 64 * n) / (128 * n)) : 0;
}

// Line-drawing bits (include/rendernet_hip.h, rn_raycast_edges_fwd).  The 16x16 tile and its line_radius halo, at most
// 24x24 pixels, are staged once: per pixel the hit voxel packed as x | y << 8 | z << 16 (kEdgeMiss for a miss, kEdgeOutside
// for a pixel outside the call's window) and the integer normal of source_normal as three 16-bit components.  After the
// barrier every hit pixel compares itself with its window out of LDS.  Every thread reaches both barriers; lanes outside the
// window stay in with nothing to write.  No float anywhere.
constexpr int kEdgeMaxRadius = 4;
constexpr int kEdgeMiss = -1, kEdgeOutside = -2;

template <bool LDS>
__global__ __launch_bounds__(256)
void raycast_edges_kernel(const unsigned* __restrict__ bits, const int* __restrict__ box, const int* __restrict__ hit_id,
                          const signed char* __restrict__ face_in, unsigned char* __restrict__ edge, int S, int ph, int pw,
                          int R, int lr, int depth_gap, int crease_q)
{
    constexpr int W = kTile + 2 * kEdgeMaxRadius;
    __shared__ unsigned slab[LDS ? kLdsWords : 1];
    __shared__ int cell_v[W * W];
    __shared__ short4 cell_n[W * W];
    const int b = blockIdx.z;
    int lo[3], hi[3];
    Occ<LDS> occ;
    open_item<LDS>(bits + (size_t)b * (S * S * (S / 32)), box + b * 6, S, slab, lo, hi, occ);

    const int r0 = blockIdx.y * kTile - lr, c0 = blockIdx.x * kTile - lr, w = kTile + 2 * lr;
    const int* hsrc = hit_id + (size_t)b * ph * pw;
    const signed char* fsrc = face_in + (size_t)b * ph * pw;
    for (int i = threadIdx.x; i < w * w; i += 256) {
        const int y = i / w, x = i - y * w, gr = r0 + y, gc = c0 + x;
        int v = kEdgeOutside;
        short4 n = make_short4(0, 0, 0, 0);
        if (gr >= 0 && gr < ph && gc >= 0 && gc < pw) {
            const int h = hsrc[(size_t)gr * pw + gc], fc = fsrc[(size_t)gr * pw + gc];
            v = kEdgeMiss;
            if (h >= 0 && h < S * S * S && fc >= 0 && fc < 6) {
                const int vx = h % S, vy = (h / S) % S, vz = h / (S * S);
                int ns[3];
                source_normal<LDS>(occ, vx, vy, vz, fc, R, ns);
                v = vx | (vy << 8) | (vz << 16);
                n = make_short4((short)ns[0], (short)ns[1], (short)ns[2], 0);
            }
        }
        cell_v[y * W + x] = v;
        cell_n[y * W + x] = n;
    }
    __syncthreads();

    const int ty = threadIdx.x / kTile, tx = threadIdx.x % kTile;
    const int pr = blockIdx.y * kTile + ty, pc = blockIdx.x * kTile + tx;
    if (pr >= ph || pc >= pw) return;                       // after the last barrier
    const int vp = cell_v[(ty + lr) * W + tx + lr];
    int out = 0;
    if (vp >= 0) {
        const short4 np = cell_n[(ty + lr) * W + tx + lr];
        const int px = vp & 255, py = (vp >> 8) & 255, pz = vp >> 16;
        const long long pp = (long long)((int)np.x * np.x + (int)np.y * np.y + (int)np.z * np.z);
        for (int dy = 0; dy <= 2 * lr; ++dy) {
            for (int dx = 0; dx <= 2 * lr; ++dx) {
                const int vq = cell_v[(ty + dy) * W + tx + dx];
                if (vq == kEdgeOutside || (dy == lr && dx == lr)) continue;
                if (vq == kEdgeMiss) { out |= 1; continue; }
                const int gap = max(max(abs(px - (vq & 255)), abs(py - ((vq >> 8) & 255))), abs(pz - (vq >> 16)));
                if (gap > depth_gap) out |= 2;
                if (!(out & 4)) {
                    const short4 nq = cell_n[(ty + dy) * W + tx + dx];
                    const int d = (int)np.x * nq.x + (int)np.y * nq.y + (int)np.z * nq.z;
                    const long long qq = (long long)((int)nq.x * nq.x + (int)nq.y * nq.y + (int)nq.z * nq.z);
                    if (d <= 0 || 8ll * d * d < (long long)crease_q * pp * qq) out |= 4;
                }
            }
        }
    }
    edge[((size_t)b * ph + pr) * pw + pc] = (unsigned char)out;
}

// The bytes of the two line pictures (include/rendernet_hip.h, rn_lines_encode), four pixels per thread: with VEC the
// twelve normal bytes, the four edge bytes and the four output bytes move as words (the pixel count is then a multiple of
// four and the three planes are 4-byte aligned).
__device__ __forceinline__ unsigned lines_byte(unsigned b0, unsigned b1, unsigned b2, unsigned e, int edge_mask, int K,
                                               int shadow, int lx, int ly, int lz)
{
    if ((b0 | b1 | b2) == 0u) return 255u;                  // a miss: white
    if (e & (unsigned)edge_mask) return 0u;                 // ink
    if (K == 0) return 255u;
    const int d = lx * (2 * (int)b0 - 255) + ly * (2 * (int)b1 - 255) + lz * (2 * (int)b2 - 255);
    const int band = min(K - 1, (K * max(d, 0)) / (32767 * 255));
    return (unsigned)(shadow + ((255 - shadow) * 2 * band + (K - 1)) / (2 * (K - 1)));
}

template <bool VEC>
__global__ __launch_bounds__(256)
void lines_encode_kernel(const unsigned char* __restrict__ normals, const unsigned char* __restrict__ edge,
                         unsigned char* __restrict__ out, size_t pixels, int edge_mask, int K, int shadow, int lx, int ly,
                         int lz)
{
    const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= pixels) return;
    if (VEC) {
        const unsigned* n4 = reinterpret_cast<const unsigned*>(normals + p0 * 3);
        const unsigned w0 = n4[0], w1 = n4[1], w2 = n4[2];
        const unsigned e4 = *reinterpret_cast<const unsigned*>(edge + p0);
        const unsigned nb[12] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, w0 >> 24, w1 & 255u, (w1 >> 8) & 255u,
                                 (w1 >> 16) & 255u, w1 >> 24, w2 & 255u, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24};
        unsigned o4 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o4 |= lines_byte(nb[3 * j], nb[3 * j + 1], nb[3 * j + 2], (e4 >> (8 * j)) & 255u, edge_mask, K, shadow, lx, ly, lz)
                  << (8 * j);
        *reinterpret_cast<unsigned*>(out + p0) = o4;
    } else {
        for (size_t p = p0; p < min(p0 + 4, pixels); ++p)
            out[p] = (unsigned char)lines_byte(normals[p * 3], normals[p * 3 + 1], normals[p * 3 + 2], edge[p], edge_mask, K,
                                               shadow, lx, ly, lz);
    }
}

// The direction to the light per item in source-grid coordinates, quantised (include/rendernet_hip.h, rn_shadow_light):
// D = rint(1023 d / max|d|) with d = M_lin w, w = the light as a camera-grid vector.  One thread per item.
constexpr int kShadowOne = 1023;

__global__ void shadow_light_kernel(const float* __restrict__ m_inv, float w0, float w1, float w2, int* __restrict__ light_src,
                                    int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* M = m_inv + (size_t)b * 12;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (M[4 * k] * w0 + M[4 * k + 1] * w1) + M[4 * k + 2] * w2;
    const float m = fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2]));
    const bool ok = isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && m > 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) light_src[b * 3 + k] = ok ? (int)rintf((float)kShadowOne * (d[k] / m)) : 0;
}

// Cast shadows of the hit faces (include/rendernet_hip.h, rn_raycast_shadow_fwd): same tile mapping and slab as
// raycast_kernel, one thread per pixel.  The shadow ray leaves the centre of the entry face along the item's integer light
// direction D and is walked in doubled integer coordinates: the next crossing of axis k is num_k / |D_k| with
// num_k = |2 u_k + sgn(D_k) - C_k|, compared by cross-multiplication (num <= 2S + 1, |D| <= 1023: below 2^20).  No float.
// Every thread reaches open_item's barrier; lanes outside the window, and misses, have nothing to walk.
template <bool LDS>
__global__ __launch_bounds__(256)
void raycast_shadow_kernel(const unsigned* __restrict__ bits, const int* __restrict__ box, const int* __restrict__ hit_id,
                           const signed char* __restrict__ face_in, const int* __restrict__ light_src,
                           unsigned char* __restrict__ lit, int S, int ph, int pw, int bias)
{
    __shared__ unsigned slab[LDS ? kLdsWords : 1];
    const int b = blockIdx.z;
    int lo[3], hi[3];
    Occ<LDS> occ;
    open_item<LDS>(bits + (size_t)b * (S * S * (S / 32)), box + b * 6, S, slab, lo, hi, occ);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pr = blockIdx.y * kTile + (wave >> 1) * 8 + (lane >> 3);
    const int pc = blockIdx.x * kTile + (wave & 1) * 8 + (lane & 7);
    if (pr >= ph || pc >= pw) return;                       // after the only barrier
    const size_t px = ((size_t)b * ph + pr) * pw + pc;

    int out = 255;
    const int h = hit_id[px], fc = face_in[px];
    if (h >= 0 && h < S * S * S && fc >= 0 && fc < 6) {
        const int a = fc >> 1, s = (fc & 1) ? 1 : -1;
        int D[3], sg[3], ad[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            D[k] = min(max(light_src[b * 3 + k], -kShadowOne), kShadowOne);
            sg[k] = D[k] > 0 ? 1 : -1;
            ad[k] = abs(D[k]);
        }
        out = 0;
        if (s * (a == 0 ? D[0] : a == 1 ? D[1] : D[2]) > 0) {
            const int v[3] = {h % S, (h / S) % S, h / (S * S)};
            int u[3], C[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                u[k] = v[k] + (k == a ? s : 0);
                C[k] = 2 * v[k] + (k == a ? s : 0);
            }
            out = 1;                                        // a ray leaves the box within 3S steps: the bound is never reached
            for (int step = 0; step < 3 * S + 3; ++step) {
                if (u[0] < lo[0] || u[0] > hi[0] || u[1] < lo[1] || u[1] > hi[1] || u[2] < lo[2] || u[2] > hi[2]) break;   // lit
                if (occ.at(u[0], u[1], u[2]) &&
                    max(max(abs(u[0] - v[0]), abs(u[1] - v[1])), abs(u[2] - v[2])) > bias) { out = 0; break; }
                int m = -1, bn = 0, bd = 1;                 // the stepping axis, its num and its |D|
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int num = abs(2 * u[k] + sg[k] - C[k]);
                    if (ad[k] != 0 && (m < 0 || num * bd < bn * ad[k])) { m = k; bn = num; bd = ad[k]; }
                }
                if (m == 0) u[0] += sg[0]; else if (m == 1) u[1] += sg[1]; else u[2] += sg[2];   // D_a != 0: m >= 0
            }
        }
    }
    lit[px] = (unsigned char)out;
}

// The bytes of the shadow picture (include/rendernet_hip.h, rn_shadow_encode): the masked mean of lit over the pixel window
// (window_sum) with (lit | 1 << 16) per hit pixel, 0 per miss (at most 289 hits), times the diffuse term of the normal bytes
// under the quantised light.
__global__ __launch_bounds__(256)
void shadow_encode_kernel(const unsigned char* __restrict__ normals, const unsigned char* __restrict__ lit,
                          unsigned char* __restrict__ out, int ph, int pw, int r, int ambient, int lx, int ly, int lz)
{
    __shared__ WindowCells<int> cell;
    __shared__ WindowRowSums<int> rowsum;
    const int b = blockIdx.z;
    const unsigned char* src = lit + (size_t)b * ph * pw;
    const auto load = [=](int gr, int gc) {
        const int cval = src[(size_t)gr * pw + gc];
        return cval <= 1 ? (cval | (1 << 16)) : 0;
    };
    int sum, centre;
    if (!window_sum<HaloLoad::clamped>(cell, rowsum, ph, pw, r, load, sum, centre)) return;   // after both barriers
    const int pr = blockIdx.y * kTile + threadIdx.x / kTile, pc = blockIdx.x * kTile + threadIdx.x % kTile;
    const int total = sum & 0xffff, n = sum >> 16;
    const size_t px = ((size_t)b * ph + pr) * pw + pc;
    int byte = 0;
    if (centre != 0) {                                      // a hit: n >= 1
        const int e = max(lx * (2 * (int)normals[px * 3] - 255) + ly * (2 * (int)normals[px * 3 + 1] - 255) +
                          lz * (2 * (int)normals[px * 3 + 2] - 255), 0);
        const long long den = 32767ll * 255ll * n;
        byte = min(255, ambient + (int)(((long long)(255 - ambient) * e * total + den / 2) / den));
    }
    out[px] = (unsigned char)byte;
}

}  // namespace

extern "C" int rn_voxel_pack(const void* vox, int vox_is_u8, float threshold, unsigned* bits, int* box, int B, int S,
                             void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_grid_side_x32(__func__, S)) return RN_E_INVALID;
    if (vox_is_u8 != 0 && vox_is_u8 != 1) return rn_set_error(RN_E_INVALID, "rn_voxel_pack: vox_is_u8=%d", vox_is_u8);
    if (!(threshold == threshold)) return rn_set_error(RN_E_INVALID, "rn_voxel_pack: threshold is NaN");
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {vox, bits, box})) return RN_E_INVALID;
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
    if (rn_check_batch_sign(__func__, B) || rn_check_grid_side_x32(__func__, S)) return RN_E_INVALID;
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
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {bits, box, m_inv, out_u8})) return RN_E_INVALID;
    if (((uintptr_t)bits & 15) != 0 || ((uintptr_t)box & 3) != 0 || ((uintptr_t)m_inv & 3) != 0 || ((uintptr_t)hit_id & 3) != 0)
        return rn_set_error(RN_E_INVALID, "rn_raycast_fwd: bits must be 16-byte aligned, box, m_inv and hit_id 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = rn_tile_grid(B, ph, pw);
    const auto kernel = S <= 64 ? raycast_kernel<true> : raycast_kernel<false>;      // the mask in LDS, or read from memory
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, bits, box, m_inv, out_u8, hit_id, face, S, N, f, row0, col0, ph, pw,
                       normal_radius, view_from_low_x);
    return rn_check_launch("rn_raycast_fwd");
}

extern "C" int rn_raycast_ao_fwd(const unsigned* bits, const int* box, const int* hit_id, const signed char* face,
                                 unsigned char* count, int B, int S, int ph, int pw, int max_distance, void* stream)
{
    static_assert(RN_AO_DIRS_COUNT == RN_AO_RAYS && RN_AO_RAYS == 64, "one ray per lane of a 64-lane wave");
    if (rn_check_batch_sign(__func__, B) || rn_check_grid_side_x32(__func__, S) || rn_check_window(__func__, ph, pw))
        return RN_E_INVALID;
    if (max_distance < 1 || max_distance > RN_AO_MAX_DISTANCE)
        return rn_set_error(RN_E_INVALID, "rn_raycast_ao_fwd: max_distance=%d (1..%d)", max_distance, RN_AO_MAX_DISTANCE);
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {bits, box, hit_id, face, count}) ||
        rn_check_hit_alignment(__func__, bits, box, hit_id))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = rn_tile_grid(B, ph, pw);
    const auto kernel = S <= 64 ? raycast_ao_kernel<true> : raycast_ao_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, bits, box, hit_id, face, count, S, ph, pw, max_distance);
    return rn_check_launch("rn_raycast_ao_fwd");
}

extern "C" int rn_ao_encode(const unsigned char* count, unsigned char* out_u8, int B, int ph, int pw, int smooth, void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_window(__func__, ph, pw) || rn_check_smooth(__func__, smooth))
        return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {count, out_u8})) return RN_E_INVALID;
    if (count == out_u8) return rn_set_error(RN_E_INVALID, "rn_ao_encode: count and out_u8 must not be the same buffer");
    hipLaunchKernelGGL(ao_encode_kernel, rn_tile_grid(B, ph, pw), dim3(256), 0, (hipStream_t)stream, count, out_u8, ph, pw,
                       smooth);
    return rn_check_launch("rn_ao_encode");
}

extern "C" int rn_raycast_edges_fwd(const unsigned* bits, const int* box, const int* hit_id, const signed char* face,
                                    unsigned char* edge, int B, int S, int ph, int pw, int normal_radius, int line_radius,
                                    int depth_gap, int crease_q, void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_grid_side_x32(__func__, S) || rn_check_window(__func__, ph, pw))
        return RN_E_INVALID;
    if (normal_radius < 1 || normal_radius > 3)
        return rn_set_error(RN_E_INVALID, "rn_raycast_edges_fwd: normal_radius=%d (1..3)", normal_radius);
    if (line_radius < 1 || line_radius > kEdgeMaxRadius)
        return rn_set_error(RN_E_INVALID, "rn_raycast_edges_fwd: line_radius=%d (1..%d)", line_radius, kEdgeMaxRadius);
    if (depth_gap < 1 || depth_gap > 127)
        return rn_set_error(RN_E_INVALID, "rn_raycast_edges_fwd: depth_gap=%d (1..127)", depth_gap);
    if (crease_q < 0 || crease_q > 8) return rn_set_error(RN_E_INVALID, "rn_raycast_edges_fwd: crease_q=%d (0..8)", crease_q);
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {bits, box, hit_id, face, edge}) ||
        rn_check_hit_alignment(__func__, bits, box, hit_id))
        return RN_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = rn_tile_grid(B, ph, pw);
    const auto kernel = S <= 64 ? raycast_edges_kernel<true> : raycast_edges_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, bits, box, hit_id, face, edge, S, ph, pw, normal_radius, line_radius,
                       depth_gap, crease_q);
    return rn_check_launch("rn_raycast_edges_fwd");
}

extern "C" int rn_lines_encode(const unsigned char* normals_u8, const unsigned char* edge, unsigned char* out_u8, int B, int ph,
                               int pw, int edge_mask, int levels, int shadow_byte, int lx, int ly, int lz, void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_window(__func__, ph, pw)) return RN_E_INVALID;
    if (edge_mask < 1 || edge_mask > 7) return rn_set_error(RN_E_INVALID, "rn_lines_encode: edge_mask=%d (1..7)", edge_mask);
    if (levels != 0 && (levels < 2 || levels > 8))
        return rn_set_error(RN_E_INVALID, "rn_lines_encode: levels=%d (0, or 2..8)", levels);
    if (shadow_byte < 0 || shadow_byte > 254)
        return rn_set_error(RN_E_INVALID, "rn_lines_encode: shadow_byte=%d (0..254)", shadow_byte);
    if (rn_check_quantised_light(__func__, lx, ly, lz)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {normals_u8, edge, out_u8})) return RN_E_INVALID;
    if (out_u8 == edge || out_u8 == normals_u8)
        return rn_set_error(RN_E_INVALID, "rn_lines_encode: out_u8 must not be one of the input buffers");
    const size_t pixels = (size_t)B * ph * pw;
    const bool vec = pixels % 4 == 0 && (((uintptr_t)normals_u8 | (uintptr_t)edge | (uintptr_t)out_u8) & 3) == 0;
    const dim3 grid((unsigned)((pixels + 1023) / 1024));
    if (vec)
        hipLaunchKernelGGL(lines_encode_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, normals_u8, edge, out_u8, pixels,
                           edge_mask, levels, shadow_byte, lx, ly, lz);
    else
        hipLaunchKernelGGL(lines_encode_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, normals_u8, edge, out_u8, pixels,
                           edge_mask, levels, shadow_byte, lx, ly, lz);
    return rn_check_launch("rn_lines_encode");
}

extern "C" int rn_shadow_light(const float* m_inv, const float* light, int view_from_low_x, int* light_src, int B, void* stream)
{
    if (rn_check_batch_sign(__func__, B)) return RN_E_INVALID;
    if (view_from_low_x != 0 && view_from_low_x != 1)
        return rn_set_error(RN_E_INVALID, "rn_shadow_light: view_from_low_x=%d", view_from_low_x);
    if (rn_check_pointers(__func__, {light})) return RN_E_INVALID;
    const float l0 = light[0], l1 = light[1], l2 = light[2];           // right, up, towards the camera; on the host
    if (!(l0 - l0 == 0.0f && l1 - l1 == 0.0f && l2 - l2 == 0.0f) || (l0 == 0.0f && l1 == 0.0f && l2 == 0.0f))
        return rn_set_error(RN_E_INVALID, "rn_shadow_light: light (%g, %g, %g), three finite numbers, not all zero", (double)l0,
                            (double)l1, (double)l2);
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {m_inv, light_src})) return RN_E_INVALID;
    if (((uintptr_t)m_inv & 3) != 0 || ((uintptr_t)light_src & 3) != 0)
        return rn_set_error(RN_E_INVALID, "rn_shadow_light: m_inv and light_src must be 4-byte aligned");
    hipLaunchKernelGGL(shadow_light_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m_inv,
                       view_from_low_x ? -l2 : l2, l1, l0, light_src, B);
    return rn_check_launch("rn_shadow_light");
}

extern "C" int rn_raycast_shadow_fwd(const unsigned* bits, const int* box, const int* hit_id, const signed char* face,
                                     const int* light_src, unsigned char* lit, int B, int S, int ph, int pw, int bias,
                                     void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_grid_side_x32(__func__, S) || rn_check_window(__func__, ph, pw))
        return RN_E_INVALID;
    if (bias < 0 || bias > 3) return rn_set_error(RN_E_INVALID, "rn_raycast_shadow_fwd: bias=%d (0..3)", bias);
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {bits, box, hit_id, face, light_src, lit}))
        return RN_E_INVALID;
    if (((uintptr_t)bits & 15) != 0 || ((uintptr_t)box & 3) != 0 || ((uintptr_t)hit_id & 3) != 0 || ((uintptr_t)light_src & 3) != 0)
        return rn_set_error(RN_E_INVALID,
                            "rn_raycast_shadow_fwd: bits must be 16-byte aligned, box, hit_id and light_src 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = rn_tile_grid(B, ph, pw);
    const auto kernel = S <= 64 ? raycast_shadow_kernel<true> : raycast_shadow_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, bits, box, hit_id, face, light_src, lit, S, ph, pw, bias);
    return rn_check_launch("rn_raycast_shadow_fwd");
}

extern "C" int rn_shadow_encode(const unsigned char* normals_u8, const unsigned char* lit, unsigned char* out_u8, int B, int ph,
                                int pw, int smooth, int ambient_byte, int lx, int ly, int lz, void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_window(__func__, ph, pw) || rn_check_smooth(__func__, smooth))
        return RN_E_INVALID;
    if (ambient_byte < 0 || ambient_byte > 254)
        return rn_set_error(RN_E_INVALID, "rn_shadow_encode: ambient_byte=%d (0..254)", ambient_byte);
    if (rn_check_quantised_light(__func__, lx, ly, lz)) return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {normals_u8, lit, out_u8})) return RN_E_INVALID;
    if (out_u8 == lit || out_u8 == normals_u8)
        return rn_set_error(RN_E_INVALID, "rn_shadow_encode: out_u8 must not be one of the input buffers");
    hipLaunchKernelGGL(shadow_encode_kernel, rn_tile_grid(B, ph, pw), dim3(256), 0, (hipStream_t)stream, normals_u8, lit, out_u8,
                       ph, pw, smooth, ambient_byte, lx, ly, lz);
    return rn_check_launch("rn_shadow_encode");
}
