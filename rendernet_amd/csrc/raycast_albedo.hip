// Albedo of the ray-cast surface: a seeded linear colour field over the voxel lattice, as 8-bit training targets for the
// texture net (gfx950).  The picture is a deterministic INTEGER function of (hit voxel, wave table, quantised texture
// code); the rule is stated in include/rendernet_hip.h (rn_raycast_albedo_fwd), the NumPy twin is
// tests/raycast_albedo_ref.py.  No float appears in this file.
//
//   rn_raycast_albedo_fwd  one thread per pixel, a 256-thread block is a 16x16 pixel tile of one item (the second-stage
//                    layout of raycast.hip).  Staged in LDS once per block: the wave table, one 128-bit read per wave,
//                    already multiplied by the item's code (q_k * amp_kc), and the 256-entry cosine.  Every lane of a wavefront
//                    reads the same wave row (an LDS broadcast) and its own cosine entry.
//   rn_albedo_encode a masked integer mean of the colours over a pixel window: ao_encode_kernel's tile + halo staging, row
//                    sums then column sums, with the three channel sums and the hit count packed in one 64-bit word.
// The arguments are checked in capi.hip; the launchers below trust them.
#include "rn_common.h"
#include "cos_q.h"

namespace {

constexpr int kTile = 16;                 // pixel tile side of one 256-thread block
constexpr int kMaxSmooth = RN_ALBEDO_MAX_SMOOTH;

__global__ __launch_bounds__(256)
void raycast_albedo_kernel(const int* __restrict__ hit_id, const uint4* __restrict__ waves, const signed char* __restrict__ code_q,
                           unsigned char* __restrict__ out, int S, int K, int ph, int pw, int base_r, int base_g, int base_b)
{
    static_assert(RN_COS_Q_COUNT == 256 && RN_ALBEDO_MAX_WAVES == 256, "one table entry and at most one wave per thread");
    __shared__ int4 wf[RN_ALBEDO_MAX_WAVES];                // fx, fy, fz, phase
    __shared__ int4 wa[RN_ALBEDO_MAX_WAVES];                // q aR, q aG, q aB, 0
    __shared__ int cosq[RN_COS_Q_COUNT];
    const int b = blockIdx.z, t = threadIdx.x;
    cosq[t] = rn_cos_q[t];
    if (t < K) {
        const uint4 w = waves[t];                           // int16 x 8, little endian: (fx fy) (fz phase) (aR aG) (aB 0)
        const int q = code_q[(size_t)b * K + t];
        wf[t] = make_int4((short)(w.x & 0xffffu), (short)(w.x >> 16), (short)(w.y & 0xffffu), (short)(w.y >> 16));
        wa[t] = make_int4(q * (short)(w.z & 0xffffu), q * (short)(w.z >> 16), q * (short)(w.w & 0xffffu), 0);
    }
    __syncthreads();
    const int pr = blockIdx.y * kTile + t / kTile, pc = blockIdx.x * kTile + t % kTile;
    if (pr >= ph || pc >= pw) return;
    const size_t px = ((size_t)b * ph + pr) * pw + pc;
    const int id = hit_id[px];
    int r = 0, g = 0, bl = 0;                               // a miss is black
    if (id >= 0 && id < S * S * S) {
        const int xs = id % S, ys = (id / S) % S, zs = id / (S * S);
        unsigned ar = 0, ag = 0, ab = 0;                    // wrap-around sums: in range for |q|, |amp| <= 127 (K 127^3 < 2^31)
        for (int k = 0; k < K; ++k) {
            const int4 f = wf[k], a = wa[k];
            const int c = cosq[(4 * (f.x * xs + f.y * ys + f.z * zs) + f.w) & 255];
            ar += (unsigned)(a.x * c);
            ag += (unsigned)(a.y * c);
            ab += (unsigned)(a.z * c);
        }
        r = min(max(base_r + ((int)(ar + 32768u) >> 16), 0), 255);
        g = min(max(base_g + ((int)(ag + 32768u) >> 16), 0), 255);
        bl = min(max(base_b + ((int)(ab + 32768u) >> 16), 0), 255);
    }
    out[px * 3] = (unsigned char)r;
    out[px * 3 + 1] = (unsigned char)g;
    out[px * 3 + 2] = (unsigned char)bl;
}

// Per hit pixel R | G << 17 | B << 34 | 1 << 51, 0 per miss or pixel outside the call: a window holds at most 289 pixels, so a
// channel sum stays below 289 * 255 < 2^17 and the count below 2^9.  Every thread reaches both barriers.
__global__ __launch_bounds__(256)
void albedo_encode_kernel(const unsigned char* __restrict__ colour, const int* __restrict__ hit_id, unsigned char* __restrict__ out,
                          int S, int ph, int pw, int r)
{
    constexpr int W = kTile + 2 * kMaxSmooth;
    __shared__ unsigned long long cell[W][W + 1];
    __shared__ unsigned long long rowsum[W][kTile];
    const int b = blockIdx.z, r0 = blockIdx.y * kTile - r, c0 = blockIdx.x * kTile - r, w = kTile + 2 * r;
    const size_t item = (size_t)b * ph * pw;
    for (int i = threadIdx.x; i < w * w; i += 256) {
        const int y = i / w, x = i - y * w, gr = r0 + y, gc = c0 + x;
        unsigned long long v = 0;
        if (gr >= 0 && gr < ph && gc >= 0 && gc < pw) {
            const size_t px = item + (size_t)gr * pw + gc;
            const int id = hit_id[px];
            if (id >= 0 && id < S * S * S)
                v = (unsigned long long)colour[px * 3] | (unsigned long long)colour[px * 3 + 1] << 17 |
                    (unsigned long long)colour[px * 3 + 2] << 34 | 1ull << 51;
        }
        cell[y][x] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < w * kTile; i += 256) {
        const int y = i / kTile, x = i % kTile;
        unsigned long long sum = 0;
        for (int dx = 0; dx <= 2 * r; ++dx) sum += cell[y][x + dx];
        rowsum[y][x] = sum;
    }
    __syncthreads();
    const int ty = threadIdx.x / kTile, tx = threadIdx.x % kTile;
    const int pr = blockIdx.y * kTile + ty, pc = blockIdx.x * kTile + tx;
    if (pr >= ph || pc >= pw) return;
    unsigned long long sum = 0;
    for (int dy = 0; dy <= 2 * r; ++dy) sum += rowsum[ty + dy][tx];
    const size_t px = item + (size_t)pr * pw + pc;
    int cr = 0, cg = 0, cb = 0;
    if (cell[ty + r][tx + r] != 0) {                        // a hit: n >= 1
        const int n = (int)(sum >> 51);
        cr = (2 * (int)(sum & 0x1ffff) + n) / (2 * n);
        cg = (2 * (int)((sum >> 17) & 0x1ffff) + n) / (2 * n);
        cb = (2 * (int)((sum >> 34) & 0x1ffff) + n) / (2 * n);
    }
    out[px * 3] = (unsigned char)cr;
    out[px * 3 + 1] = (unsigned char)cg;
    out[px * 3 + 2] = (unsigned char)cb;
}

}  // namespace

int rn_launch_raycast_albedo(const int* hit_id, const short* waves, const signed char* code_q, const int* base,
                             unsigned char* out_u8, int B, int S, int K, int ph, int pw, hipStream_t st)
{
    const dim3 grid((unsigned)((pw + kTile - 1) / kTile), (unsigned)((ph + kTile - 1) / kTile), (unsigned)B);
    hipLaunchKernelGGL(raycast_albedo_kernel, grid, dim3(256), 0, st, hit_id, (const uint4*)waves, code_q, out_u8, S, K, ph, pw,
                       base[0], base[1], base[2]);
    return rn_check_launch("rn_raycast_albedo_fwd");
}

int rn_launch_albedo_encode(const unsigned char* colour, const int* hit_id, unsigned char* out_u8, int B, int S, int ph, int pw,
                            int smooth, hipStream_t st)
{
    const dim3 grid((unsigned)((pw + kTile - 1) / kTile), (unsigned)((ph + kTile - 1) / kTile), (unsigned)B);
    hipLaunchKernelGGL(albedo_encode_kernel, grid, dim3(256), 0, st, colour, hit_id, out_u8, S, ph, pw, smooth);
    return rn_check_launch("rn_albedo_encode");
}
