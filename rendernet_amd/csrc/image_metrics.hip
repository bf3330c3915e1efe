// Image-quality metrics of two image batches on the device: the sums behind L1 / PSNR and the windowed SSIM sum (gfx950).
// Both images are compared as BYTES (a float image is quantised while it is staged), every moment is an integer and the
// only floating-point step is the float64 SSIM quotient; the rule, its weights and the bounds that keep every intermediate
// inside 32 / 64 bits are stated in include/rendernet_hip.h (rn_image_metrics), the NumPy twin is tests/image_metrics_ref.py.
// Built with -ffp-contract=off: 2 A B and A A + B B must round the same way, so that equal images give exactly 1.0.
//
//   image_metrics_tile_kernel   a 256-thread block takes a tile of 16 rows x 64 SAMPLES of one image, a sample being one
//                    channel of one pixel in memory order.  A row [W,C] is a flat array of W C samples and the window of
//                    sample s reads the samples s + d C, d = 0..10, so all channels go through one code path with a tap stride
//                    of C, and the global reads of an interleaved C = 3 image are whole contiguous rows (a block per channel
//                    would fetch every line three times and use a third of it).  Stage 26 x (64 + 10 C) bytes of each image in
//                    LDS (quantising floats; samples outside the image are 0 and feed only windows that are masked out); the
//                    horizontal pass writes the five moments of each staged row as 32-bit words (4096 * 65025 < 2^32); the
//                    vertical pass gives a thread one column and 4 output rows, A and B in 32 bits, the second moments with
//                    64-bit multiply-adds; then the central moments, the float64 quotient, and a block sum in a fixed order.
//                    sad / ssd: every pixel of the image belongs to exactly one tile (a tile owns its 16 x 64 samples, the last
//                    tile of a row or column also the halo beyond them) and is counted while it is staged.
//                    The tile is this small for occupancy: 38 KB of LDS lets four blocks share a CU, and with barriers between
//                    the phases it is the other blocks that hide a block's staging loads (measured: DESIGN.md, Validation metrics).
//   image_metrics_sum_kernel    one block per image adds the tiles' partial sums in a fixed order: no floating-point atomics, the
//                    same inputs give the same bits on every call.
#include "voxel_common.h"
#include "rn_checks.h"

namespace {

constexpr int kTH = 16;                           // output rows of a tile
constexpr int kTW = 64;                           // output samples of a tile
constexpr int kHalo = 10;                         // window 11: ten more rows, ten more pixels
constexpr int kRows = kTH + kHalo;
constexpr int kRowsPerThread = 4;                 // vertical pass: 64 columns x 4 row groups = 256 threads
constexpr unsigned kT = 1u << 24;                 // total 2-D weight
static_assert(kTW * (kTH / kRowsPerThread) == 256, "one column and one row group per thread");

struct Partial { double ssim; long long sad, ssd; };          // per tile; RN_METRICS_PARTIAL_BYTES
static_assert(sizeof(Partial) == RN_METRICS_PARTIAL_BYTES, "workspace stride");

__device__ __forceinline__ unsigned quantise(float x)
{
    float v = 255.f * x;
    v = v > 0.f ? v : 0.f;                        // a NaN fails the comparison: 0
    v = v < 255.f ? v : 255.f;
    return (unsigned)rintf(v);                    // half to even
}

__device__ __forceinline__ unsigned load_byte(const void* p, size_t i, int is_f32)
{
    return is_f32 ? quantise(((const float*)p)[i]) : (unsigned)((const unsigned char*)p)[i];
}

template <int C>
__global__ __launch_bounds__(256)
void image_metrics_tile_kernel(const void* __restrict__ a, const void* __restrict__ b, int a_f32, int b_f32, int H, int W,
                               Partial* __restrict__ part)
{
    constexpr int kSW = kTW + kHalo * C;                      // staged samples of a row
    constexpr int kSWp = (kSW + 3) & ~3;
    constexpr int kWt[11] = {RN_SSIM_WEIGHTS};
    constexpr int kND = (4 + kHalo * C + 3) / 4;               // dwords that hold the bytes of four neighbouring windows
    static_assert(kTW - 4 + 4 * kND <= kSWp, "the last quad's dwords end inside the padded row");
    __shared__ __attribute__((aligned(16))) unsigned char sa[kRows][kSWp], sb[kRows][kSWp];
    __shared__ __attribute__((aligned(16))) unsigned hm[5][kRows][kTW];
    __shared__ double redd[4];
    __shared__ unsigned redu[4];

    const int t = threadIdx.x;
    const int WC = W * C, row0 = blockIdx.y * kTH, col0 = blockIdx.x * kTW;
    const bool lastx = blockIdx.x == gridDim.x - 1, lasty = blockIdx.y == gridDim.y - 1;
    const size_t img = (size_t)blockIdx.z * H * WC;

    unsigned sad = 0, ssd = 0;                                // a tile stages 26 * 94 samples: 255^2 times that is below 2^28
    for (int i = t; i < kRows * kSW; i += 256) {
        const int r = i / kSW, j = i - r * kSW;
        const int row = row0 + r, col = col0 + j;
        unsigned va = 0, vb = 0;
        if (row < H && col < WC) {
            const size_t g = img + (size_t)row * WC + col;
            va = load_byte(a, g, a_f32);
            vb = load_byte(b, g, b_f32);
            if ((r < kTH || lasty) && (j < kTW || lastx)) {
                const int d = (int)va - (int)vb;
                sad += (unsigned)abs(d);
                ssd += (unsigned)(d * d);
            }
        }
        sa[r][j] = (unsigned char)va;
        sb[r][j] = (unsigned char)vb;
    }
    __syncthreads();

    // horizontal pass: an item is four neighbouring samples of one staged row; their windows span 4 + 10 C bytes, read as
    // whole dwords (the bytes past kSW in the last dword of a row are never selected), and each moment leaves as one 128-bit store
    for (int i = t; i < kRows * (kTW / 4); i += 256) {
        const int r = i / (kTW / 4), c0 = (i % (kTW / 4)) * 4;
        unsigned wa[kND], wb[kND];
#pragma unroll
        for (int k = 0; k < kND; ++k) {
            wa[k] = ((const unsigned*)&sa[r][c0])[k];
            wb[k] = ((const unsigned*)&sb[r][c0])[k];
        }
        uint4 m[5];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            unsigned A = 0, B = 0, Saa = 0, Sbb = 0, Sab = 0;
#pragma unroll
            for (int d = 0; d < 11; ++d) {
                const int k = o + d * C;
                const unsigned x = (wa[k >> 2] >> ((k & 3) * 8)) & 255u, y = (wb[k >> 2] >> ((k & 3) * 8)) & 255u;
                const unsigned wx = kWt[d] * x, wy = kWt[d] * y;
                A += wx; B += wy;
                Saa += wx * x; Sbb += wy * y; Sab += wx * y;
            }
            (&m[0].x)[o] = A; (&m[1].x)[o] = B; (&m[2].x)[o] = Saa; (&m[3].x)[o] = Sbb; (&m[4].x)[o] = Sab;
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) *(uint4*)&hm[q][r][c0] = m[q];
    }
    __syncthreads();

    const double c1 = RN_SSIM_K1 * 281474976710656.0, c2 = RN_SSIM_K2 * 281474976710656.0;       // times T^2 = 2^48, exact
    const int nrow = H - kHalo - row0, ncol = (W - kHalo) * C - col0;                             // valid outputs of this tile
    // vertical pass: a thread owns one column and 4 output rows; it reads the 14 staged rows under them once each and adds
    // every row into the outputs whose window holds it
    const int c = t & (kTW - 1), r0 = t / kTW * kRowsPerThread;
    unsigned mA[kRowsPerThread] = {}, mB[kRowsPerThread] = {};
    unsigned long long mSaa[kRowsPerThread] = {}, mSbb[kRowsPerThread] = {}, mSab[kRowsPerThread] = {};
#pragma unroll
    for (int j = 0; j < kRowsPerThread + kHalo; ++j) {
        const unsigned h0 = hm[0][r0 + j][c], h1 = hm[1][r0 + j][c], h2 = hm[2][r0 + j][c], h3 = hm[3][r0 + j][c], h4 = hm[4][r0 + j][c];
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            if (j - k < 0 || j - k > kHalo) continue;
            const unsigned w = kWt[j - k];
            mA[k] += w * h0;
            mB[k] += w * h1;
            mSaa[k] += (unsigned long long)w * h2;
            mSbb[k] += (unsigned long long)w * h3;
            mSab[k] += (unsigned long long)w * h4;
        }
    }
    double ssim = 0.0;
    if (c < ncol) {
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            if (r0 + k >= nrow) break;
            const unsigned A = mA[k], B = mB[k];
            const unsigned long long Saa = mSaa[k], Sbb = mSbb[k], Sab = mSab[k];
            const unsigned long long AA = (unsigned long long)A * A, BB = (unsigned long long)B * B, AB = (unsigned long long)A * B;
            const unsigned long long Va = Saa * kT - AA, Vb = Sbb * kT - BB;                     // >= 0
            const long long Cab = (long long)(Sab * kT - AB);                                     // wraps to the signed value
            const double dA = (double)A, dB = (double)B;
            const double num = (2.0 * dA * dB + c1) * (2.0 * (double)Cab + c2);
            const double den = (dA * dA + dB * dB + c1) * ((double)Va + (double)Vb + c2);
            ssim += num / den;
        }
    }
    ssim = block_sum(ssim, redd);
    sad = block_sum(sad, redu);
    ssd = block_sum(ssd, redu);
    if (t == 0) {
        Partial p;
        p.ssim = ssim; p.sad = sad; p.ssd = ssd;
        part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(256)
void image_metrics_sum_kernel(const Partial* __restrict__ part, int ntiles, long long* __restrict__ sad, long long* __restrict__ ssd,
                              double* __restrict__ ssim_sum)
{
    __shared__ double redd[4];
    __shared__ long long redl[4];
    const Partial* p = part + (size_t)blockIdx.x * ntiles;
    double s = 0.0;
    long long u = 0, v = 0;
    for (int i = threadIdx.x; i < ntiles; i += 256) { s += p[i].ssim; u += p[i].sad; v += p[i].ssd; }
    s = block_sum(s, redd);
    u = block_sum(u, redl);
    v = block_sum(v, redl);
    if (threadIdx.x == 0) { ssim_sum[blockIdx.x] = s; sad[blockIdx.x] = u; ssd[blockIdx.x] = v; }
}

inline int tiles_y(int H) { return (H - kHalo + kTH - 1) / kTH; }
inline int tiles_x(int W, int C) { return ((W - kHalo) * C + kTW - 1) / kTW; }

int check_shape(const char* who, int B, int H, int W, int C)
{
    if (rn_check_batch(who, B)) return RN_E_INVALID;
    if (C != 1 && C != 3) return rn_set_error(RN_E_INVALID, "%s: C=%d (1 or 3 channels)", who, C);
    if (H < 11 || W < 11) return rn_set_error(RN_E_INVALID, "%s: H=%d W=%d (the 11 x 11 window needs at least 11 x 11 pixels)", who, H, W);
    if (H > 32768 || W > 32768) return rn_set_error(RN_E_INVALID, "%s: H=%d W=%d (at most 32768 x 32768)", who, H, W);
    return RN_OK;
}

}  // namespace

extern "C" size_t rn_image_metrics_workspace_bytes(int B, int H, int W, int C)
{
    if (check_shape("rn_image_metrics_workspace_bytes", B, H, W, C) != RN_OK) return 0;
    return (size_t)B * tiles_y(H) * tiles_x(W, C) * sizeof(Partial);
}

extern "C" int rn_image_metrics(const void* a, int a_dtype, const void* b, int b_dtype, int B, int H, int W, int C,
                                long long* sad, long long* ssd, double* ssim_sum, void* workspace, size_t workspace_bytes,
                                void* stream)
{
    const int rc = check_shape("rn_image_metrics", B, H, W, C);
    if (rc != RN_OK) return rc;
    if ((a_dtype != RN_METRICS_U8 && a_dtype != RN_METRICS_F32) || (b_dtype != RN_METRICS_U8 && b_dtype != RN_METRICS_F32))
        return rn_set_error(RN_E_INVALID, "rn_image_metrics: dtypes %d, %d (RN_METRICS_U8 or RN_METRICS_F32)", a_dtype, b_dtype);
    if (B == 0) return RN_OK;
    // the workspace holds Partials: 8-byte aligned is enough, so this is not rn_check_ws
    if (rn_check_pointers(__func__, {a, b, sad, ssd, ssim_sum, workspace}) ||
        rn_check_aligned(__func__, a, a_dtype == RN_METRICS_F32 ? 4 : 1, "a") ||
        rn_check_aligned(__func__, b, b_dtype == RN_METRICS_F32 ? 4 : 1, "b") || rn_check_aligned(__func__, sad, 8, "sad") ||
        rn_check_aligned(__func__, ssd, 8, "ssd") || rn_check_aligned(__func__, ssim_sum, 8, "ssim_sum") ||
        rn_check_aligned(__func__, workspace, 8, "the workspace"))
        return RN_E_INVALID;
    const size_t need = rn_image_metrics_workspace_bytes(B, H, W, C);
    if (workspace_bytes < need)
        return rn_set_error(RN_E_INVALID, "rn_image_metrics: workspace of %zu bytes, %zu needed (rn_image_metrics_workspace_bytes)",
                            workspace_bytes, need);
    const int ty = tiles_y(H), tx = tiles_x(W, C);            // ty <= 2048, tx <= 1536
    const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)B);
    Partial* part = (Partial*)workspace;
    if (C == 1)
        hipLaunchKernelGGL(image_metrics_tile_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a, b, a_dtype == RN_METRICS_F32,
                           b_dtype == RN_METRICS_F32, H, W, part);
    else
        hipLaunchKernelGGL(image_metrics_tile_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a, b, a_dtype == RN_METRICS_F32,
                           b_dtype == RN_METRICS_F32, H, W, part);
    const int rl = rn_check_launch("rn_image_metrics");
    if (rl != RN_OK) return rl;
    hipLaunchKernelGGL(image_metrics_sum_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, part, ty * tx, sad, ssd, ssim_sum);
    return rn_check_launch("rn_image_metrics (sum)");
}
