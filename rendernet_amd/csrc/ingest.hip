// Target ingest: decoded 8-bit training frames -> the float32 crop the loss kernel reads (gfx950).
//
// Replaces, for frames that reach the device as bytes, the host work of the reference's loader and feed:
//   tools/data_util.py:64-157   float32 conversion, np.mean over the channels (flatten) or [:, :, :3] (colour)
//   RenderNet_Shader.py:224     images / 255.0
//   tools/model_util.py:99      the [4r:4(r+p), 4c:4(c+p)] window of the 512^2 frame
// in one pass over the window only.  The arithmetic is the host's, operation by operation: a float32 sum of the
// channels (exact, at most 1020), a float32 division by the channel count, a float32 division by 255 -- both divisions
// correctly rounded (this file is built without any fast-math flag; tests/test_gpu_ingest.py holds it to every
// possible input value).
//
// Pure streaming: per output pixel at most 4 bytes in and 4-12 bytes out.  The vector kernel gives each thread four
// pixels of one output row: 4*Cs bytes in (dword loads when the address allows, byte loads otherwise -- the same
// values either way), Co 16-byte stores out.  It needs pw % 4 == 0 and a 16-byte aligned output; anything else takes
// the one-pixel-per-thread kernel.
#include "rn_common.h"

namespace {

template <int N>
__device__ __forceinline__ void load_bytes(const unsigned char* __restrict__ p, unsigned (&v)[N])
{
    static_assert(N % 4 == 0, "whole dwords");
    if constexpr (N == 16) {
        if (((uintptr_t)p & 15) == 0) {
            const uint4 w = *reinterpret_cast<const uint4*>(p);
            const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[4 * i + k] = (ws[i] >> (8 * k)) & 255u;
            }
            return;
        }
    }
    if (((uintptr_t)p & 3) == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const unsigned w = reinterpret_cast<const unsigned*>(p)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[4 * i + k] = (w >> (8 * k)) & 255u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = p[i];
    }
}

// channel `ch` of the output pixel whose CS source bytes are s[0..CS)
template <int CS, int CO>
__device__ __forceinline__ float ingest_value(const unsigned* s, int ch)
{
    if (CO == 3 || CS == 1) return (float)s[ch] / 255.0f;
    unsigned sum = 0;
#pragma unroll
    for (int k = 0; k < CS; ++k) sum += s[k];
    return ((float)sum / (float)CS) / 255.0f;
}

// one thread = four consecutive pixels of one output row (pw % 4 == 0, patch 16-byte aligned)
template <int CS, int CO>
__global__ __launch_bounds__(256)
void ingest_vec_kernel(const unsigned char* __restrict__ frames, float* __restrict__ patch, size_t nquads,
                       int H, int W, int row0, int col0, int ph, int pw)
{
    const size_t qrow = (size_t)(pw / 4);
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nquads; q += (size_t)gridDim.x * 256) {
        const size_t orow = q / qrow;                       // b * ph + r
        const size_t c = (q - orow * qrow) * 4;             // first of the four output columns
        const size_t b = orow / (size_t)ph, r = orow - b * (size_t)ph;
        const unsigned char* src = frames + (((b * H + (size_t)row0 + r) * W) + (size_t)col0 + c) * CS;
        unsigned v[4 * CS];
        load_bytes<4 * CS>(src, v);
        float o[4 * CO];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
#pragma unroll
            for (int ch = 0; ch < CO; ++ch) o[px * CO + ch] = ingest_value<CS, CO>(v + px * CS, ch);
        }
        float4* dst = reinterpret_cast<float4*>(patch + (orow * (size_t)pw + c) * CO);
#pragma unroll
        for (int k = 0; k < CO; ++k) dst[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
}

// one thread = one pixel (any pw, any float-aligned output)
template <int CS, int CO>
__global__ __launch_bounds__(256)
void ingest_px_kernel(const unsigned char* __restrict__ frames, float* __restrict__ patch, size_t npix,
                      int H, int W, int row0, int col0, int ph, int pw)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const size_t orow = i / (size_t)pw, c = i - orow * (size_t)pw;
        const size_t b = orow / (size_t)ph, r = orow - b * (size_t)ph;
        const unsigned char* src = frames + (((b * H + (size_t)row0 + r) * W) + (size_t)col0 + c) * CS;
        unsigned s[CS];
#pragma unroll
        for (int k = 0; k < CS; ++k) s[k] = src[k];
#pragma unroll
        for (int ch = 0; ch < CO; ++ch) patch[i * CO + ch] = ingest_value<CS, CO>(s, ch);
    }
}

template <int CS, int CO>
void launch_ingest(const unsigned char* frames, float* patch, int B, int H, int W, int row0, int col0, int ph, int pw,
                   hipStream_t st)
{
    const size_t npix = (size_t)B * ph * pw;
    const bool vec = pw % 4 == 0 && ((uintptr_t)patch & 15) == 0;
    const size_t work = vec ? npix / 4 : npix;
    size_t nb = (work + 255) / 256;
    if (nb > 2048) nb = 2048;
    if (vec)
        hipLaunchKernelGGL((ingest_vec_kernel<CS, CO>), dim3((unsigned)nb), dim3(256), 0, st, frames, patch, work,
                           H, W, row0, col0, ph, pw);
    else
        hipLaunchKernelGGL((ingest_px_kernel<CS, CO>), dim3((unsigned)nb), dim3(256), 0, st, frames, patch, work,
                           H, W, row0, col0, ph, pw);
}

}  // namespace

extern "C" int rn_target_u8_crop_fwd(const unsigned char* frames, float* patch, int B, int H, int W, int Cs, int Co,
                                     int row0, int col0, int ph, int pw, void* stream)
{
    if (B < 0 || H < 1 || W < 1)
        return rn_set_error(RN_E_INVALID, "rn_target_u8_crop_fwd: B=%d H=%d W=%d", B, H, W);
    if (!((Co == 1 && (Cs == 1 || Cs == 3 || Cs == 4)) || (Co == 3 && (Cs == 3 || Cs == 4))))
        return rn_set_error(RN_E_INVALID, "rn_target_u8_crop_fwd: Cs=%d -> Co=%d (Co 1 takes Cs 1|3|4, Co 3 takes Cs 3|4)", Cs, Co);
    if (row0 < 0 || col0 < 0 || ph < 1 || pw < 1 || ph > H - row0 || pw > W - col0)
        return rn_set_error(RN_E_INVALID, "rn_target_u8_crop_fwd: window rows %d+%d cols %d+%d outside the %dx%d frame",
                            row0, ph, col0, pw, H, W);
    if (B == 0) return RN_OK;
    if (!frames || !patch) return rn_set_error(RN_E_INVALID, "rn_target_u8_crop_fwd: null pointer");
    if (((uintptr_t)patch & 3) != 0) return rn_set_error(RN_E_INVALID, "rn_target_u8_crop_fwd: patch must be float-aligned");
    hipStream_t st = (hipStream_t)stream;
    if (Co == 3) {
        if (Cs == 3) launch_ingest<3, 3>(frames, patch, B, H, W, row0, col0, ph, pw, st);
        else launch_ingest<4, 3>(frames, patch, B, H, W, row0, col0, ph, pw, st);
    } else {
        if (Cs == 1) launch_ingest<1, 1>(frames, patch, B, H, W, row0, col0, ph, pw, st);
        else if (Cs == 3) launch_ingest<3, 1>(frames, patch, B, H, W, row0, col0, ph, pw, st);
        else launch_ingest<4, 1>(frames, patch, B, H, W, row0, col0, ph, pw, st);
    }
    return rn_check_launch("rn_target_u8_crop_fwd");
}
