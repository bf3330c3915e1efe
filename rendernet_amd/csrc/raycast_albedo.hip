// Albedo of the ray-cast surface: a seeded linear colour field over the voxel lattice, as 8-bit training targets for the
// texture net (gfx950).  The picture is a deterministic INTEGER function of (hit voxel, wave table, quantised texture
// code); the rule is stated in include/rendernet_hip.h (rn_raycast_albedo_fwd), the NumPy twin is
// tests/raycast_albedo_ref.py.  No float appears in this file.
//
//   rn_raycast_albedo_fwd  one thread per pixel, a 256-thread block is a 16x16 pixel tile of one item (the second-stage
//                    layout of raycast.hip).  Staged in LDS once per block: the wave table, one 128-bit read per wave,
//                    already multiplied by the item's code (q_k * amp_kc), and the 256-entry cosine.  Every lane of a wavefront
//                    reads the same wave row (an LDS broadcast) and its own cosine entry.
//   rn_albedo_encode a masked integer mean of the colours over a pixel window (window_sum of raycast_common.h, the one of
//                    ao_encode_kernel), with the three channel sums and the hit count packed in one 64-bit word.
// The entry points below check their arguments, overlap of input and output ranges included, as those of raycast.hip do.
#include "raycast_common.h"
#include "cos_q.h"

namespace {

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
// channel sum stays below 289 * 255 < 2^17 and the count below 2^9.
__global__ __launch_bounds__(256)
void albedo_encode_kernel(const unsigned char* __restrict__ colour, const int* __restrict__ hit_id, unsigned char* __restrict__ out,
                          int S, int ph, int pw, int r)
{
    __shared__ WindowCells<unsigned long long> cell;
    __shared__ WindowRowSums<unsigned long long> rowsum;
    const int b = blockIdx.z;
    const size_t item = (size_t)b * ph * pw;
    const auto load = [=](int gr, int gc) {
        const size_t px = item + (size_t)gr * pw + gc;
        const int id = hit_id[px];
        if (id < 0 || id >= S * S * S) return 0ull;
        return (unsigned long long)colour[px * 3] | (unsigned long long)colour[px * 3 + 1] << 17 |
               (unsigned long long)colour[px * 3 + 2] << 34 | 1ull << 51;
    };
    unsigned long long sum, centre;
    if (!window_sum<HaloLoad::predicated>(cell, rowsum, ph, pw, r, load, sum, centre)) return;   // after both barriers
    const int pr = blockIdx.y * kTile + threadIdx.x / kTile, pc = blockIdx.x * kTile + threadIdx.x % kTile;
    const size_t px = item + (size_t)pr * pw + pc;
    int cr = 0, cg = 0, cb = 0;
    if (centre != 0) {                                      // a hit: n >= 1
        const int n = (int)(sum >> 51);
        cr = (2 * (int)(sum & 0x1ffff) + n) / (2 * n);
        cg = (2 * (int)((sum >> 17) & 0x1ffff) + n) / (2 * n);
        cb = (2 * (int)((sum >> 34) & 0x1ffff) + n) / (2 * n);
    }
    out[px * 3] = (unsigned char)cr;
    out[px * 3 + 1] = (unsigned char)cg;
    out[px * 3 + 2] = (unsigned char)cb;
}

// two byte ranges [a, a + na) and [b, b + nb) overlap
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int rn_raycast_albedo_fwd(const int* hit_id, const short* waves, const signed char* code_q, const int* base,
                                     unsigned char* out_u8, int B, int S, int K, int ph, int pw, void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_grid_side_x32(__func__, S)) return RN_E_INVALID;
    if (K < 1 || K > RN_ALBEDO_MAX_WAVES)
        return rn_set_error(RN_E_INVALID, "rn_raycast_albedo_fwd: K=%d (1..%d waves)", K, RN_ALBEDO_MAX_WAVES);
    if (rn_check_window(__func__, ph, pw) || rn_check_pointers(__func__, {base})) return RN_E_INVALID;
    for (int c = 0; c < 3; ++c)
        if (base[c] < 0 || base[c] > 255)
            return rn_set_error(RN_E_INVALID, "rn_raycast_albedo_fwd: base (%d, %d, %d), each 0..255", base[0], base[1], base[2]);
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {hit_id, waves, code_q, out_u8})) return RN_E_INVALID;
    if (((uintptr_t)hit_id & 3) != 0 || ((uintptr_t)waves & 15) != 0)
        return rn_set_error(RN_E_INVALID, "rn_raycast_albedo_fwd: hit_id must be 4-byte aligned, waves 16-byte aligned");
    const size_t pixels = (size_t)B * ph * pw;
    if (ranges_overlap(out_u8, pixels * 3, hit_id, pixels * 4))
        return rn_set_error(RN_E_INVALID, "rn_raycast_albedo_fwd: out_u8 must not overlap hit_id");
    hipLaunchKernelGGL(raycast_albedo_kernel, rn_tile_grid(B, ph, pw), dim3(256), 0, (hipStream_t)stream, hit_id,
                       (const uint4*)waves, code_q, out_u8, S, K, ph, pw, base[0], base[1], base[2]);
    return rn_check_launch("rn_raycast_albedo_fwd");
}

extern "C" int rn_albedo_encode(const unsigned char* colour, const int* hit_id, unsigned char* out_u8, int B, int S, int ph,
                                int pw, int smooth, void* stream)
{
    if (rn_check_batch_sign(__func__, B) || rn_check_grid_side_x32(__func__, S) || rn_check_window(__func__, ph, pw) ||
        rn_check_smooth(__func__, smooth))
        return RN_E_INVALID;
    if (B == 0) return RN_OK;
    if (rn_check_batch_size(__func__, B) || rn_check_pointers(__func__, {colour, hit_id, out_u8})) return RN_E_INVALID;
    if (((uintptr_t)hit_id & 3) != 0) return rn_set_error(RN_E_INVALID, "rn_albedo_encode: hit_id must be 4-byte aligned");
    const size_t pixels = (size_t)B * ph * pw;
    if (ranges_overlap(out_u8, pixels * 3, colour, pixels * 3) || ranges_overlap(out_u8, pixels * 3, hit_id, pixels * 4))
        return rn_set_error(RN_E_INVALID, "rn_albedo_encode: out_u8 must not overlap colour or hit_id");
    hipLaunchKernelGGL(albedo_encode_kernel, rn_tile_grid(B, ph, pw), dim3(256), 0, (hipStream_t)stream, colour, hit_id, out_u8,
                       S, ph, pw, smooth);
    return rn_check_launch("rn_albedo_encode");
}
