// The Winograd transforms and the operand split of the three-launch family (conv_wino43.hip, conv_wino43_wgrad.hip, conv_wino_bf3.hip,
// conv_wino_bf3_wgrad.hip), each stated once.  Hand-written; the matrices themselves are wino_mats.h (generated).
//
//     Y = A^T [ (G g G^T) .* (B^T d B) ] A
//
// Every function here is force-inlined into the kernel that calls it, and the loops keep one shape -- acc = 0; for k ascending:
// if (cf != 0) acc += cf * d[k], on the caller's value type.  The library builds with -ffp-contract=fast: which multiply fuses with
// which add depends on the basic blocks the optimiser leaves around it, so a kernel's bits are a property of the kernel, not of these
// functions alone.  Constraint: a kernel moves onto (or off) them only with a byte comparison of its outputs against the previous
// build.  The filter-gradient transforms (A dY A^T, G^T dU G, the tile-major B^T d B of conv_wino_bf3_wgrad.hip) do not meet it for
// F(4x4,4x4) and are written out in their kernels.
#pragma once
#include "rn_common.h"
#include "wino_mats.h"
#include <type_traits>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// XCD k (= workgroup id % 8) gets a contiguous range of the logical ids: neighbouring tiles share patch pixels / lines
__device__ __forceinline__ unsigned xcd_contiguous(unsigned blk, unsigned nblk8) { return (blk & 7u) * (nblk8 >> 3) + (blk >> 3); }

// Calls fn(S{}) with the type of a scheme id (wino_mats.h), for the schemes of SET only: WINO_CONV = the three filter schemes,
// WINO_SPLIT = those and the 1x1 plane WinoF11 (callers on the split path), WINO_M4 = the 4x4-output schemes (the filter gradients).
// false = unknown or excluded scheme, fn not called: the caller returns its own error.
enum WinoSet { WINO_M4 = 1 << RN_WINO_F43 | 1 << RN_WINO_F44, WINO_CONV = WINO_M4 | 1 << RN_WINO_F63, WINO_SPLIT = WINO_CONV | 1 << RN_WINO_F11 };

template <WinoSet SET = WINO_CONV, class Fn>
inline bool wino_with_scheme(int scheme, Fn&& fn)
{
    switch (scheme) {
    case RN_WINO_F43: if constexpr ((SET >> RN_WINO_F43 & 1) != 0) { fn(WinoF43{}); return true; } break;
    case RN_WINO_F44: if constexpr ((SET >> RN_WINO_F44 & 1) != 0) { fn(WinoF44{}); return true; } break;
    case RN_WINO_F63: if constexpr ((SET >> RN_WINO_F63 & 1) != 0) { fn(WinoF63{}); return true; } break;
    case RN_WINO_F11: if constexpr ((SET >> RN_WINO_F11 & 1) != 0) { fn(WinoF11{}); return true; } break;
    }
    return false;
}

// channels per thread of the fp32 input / output transforms: 36 x 4 | 49 x 2 | 64 x 2 registers of patch; the 1x1 plane: 4
template <class S> constexpr int wino_vw = (std::is_same_v<S, WinoF43> || std::is_same_v<S, WinoF11>) ? 4 : 2;

// ---------------------------------------------------------------------------------------------------------------------
// B^T applied to one vector of S::TA values.  BT_DENSE: row by row.  BT_FACTORED: for F(6x6,3x3) rows 1..6 come in +/- pairs over the
// even and the odd inputs, rows 0 and 7 are a difference pair each -- 26 operations where the dense form (44 non-zeros) takes 44
// (the split input transform is issue-bound: 4.7 TB/s of a 7.0 TB/s pure-write stream); every other scheme has the dense form only.
// The two are the same to rounding order, NOT to the bit: the exact-fp32 kernels are dense, the forward split kernels factored.
enum BtForm { BT_DENSE, BT_FACTORED };

template <class S, BtForm FORM, class V>
__device__ __forceinline__ void bt_apply(const V (&d)[S::TA], V (&o)[S::TA])
{
    if constexpr (FORM == BT_FACTORED && S::TA == 8 && S::R == 3) {
        o[0] = (d[6] - d[0]) + 5.25f * (d[2] - d[4]);
        o[7] = (d[7] - d[1]) + 5.25f * (d[3] - d[5]);
        const V e1 = (d[2] + d[6]) - 4.25f * d[4], f1 = (d[1] + d[5]) - 4.25f * d[3];
        o[1] = e1 + f1;
        o[2] = e1 - f1;
        const V e2 = (d[6] + 0.25f * d[2]) - 1.25f * d[4], f2 = (0.5f * d[1] - 2.5f * d[3]) + 2.f * d[5];
        o[3] = e2 + f2;
        o[4] = e2 - f2;
        const V e3 = (d[6] + 4.f * d[2]) - 5.f * d[4], f3 = (2.f * d[1] - 2.5f * d[3]) + 0.5f * d[5];
        o[5] = e3 + f3;
        o[6] = e3 - f3;
    } else {
#pragma unroll
        for (int i = 0; i < S::TA; ++i) {
            V acc = V(0.f);
#pragma unroll
            for (int k = 0; k < S::TA; ++k) {
                const float cf = S::BT(i, k);
                if (cf != 0.f) acc += cf * d[k];
            }
            o[i] = acc;
        }
    }
}

// Input transform of one tile, first half: tt[i][col] = (B^T d)[i][col] for channels c .. of tile t (V = float, f32x2 or f32x4 of
// consecutive channels); the caller finishes row i of V = B^T d B with bt_apply<S, FORM>(tt[i], ...).  !live: a zero tile, nothing is
// read.  One 64-bit multiply per thread: the A x A addresses are the tile's corner (possibly outside the plane -- then never
// dereferenced) plus offsets r W C + col C that are the same for every lane, i.e. scalar arithmetic.
template <class S, BtForm FORM, class V>
__device__ __forceinline__ void wino_input_btd(const float* x, long long t, bool live, int c, int H, int W, int C,
                                               int th, int tw, int pad_lo, V (&tt)[S::TA][S::TA])
{
    constexpr int A = S::TA;
    const long long tc = live ? t : 0;
    const int tx = (int)(tc % tw), ty = (int)((tc / tw) % th);
    const long long b = tc / ((long long)tw * th);
    const int y0 = S::M * ty - pad_lo, x0 = S::M * tx - pad_lo;
    const float* p0 = x + (((long long)b * H + y0) * W + x0) * (long long)C + (live ? c : 0);
    const long long rs = (long long)W * C;
    const float* prow[A];                                  // (A row pointers: the column step col C is then one scalar-offset add per load)
#pragma unroll
    for (int r = 0; r < A; ++r) prow[r] = r == 0 ? p0 : prow[r - 1] + rs;
#pragma unroll
    for (int col = 0; col < A; ++col) {
        V d[A];
        const bool cok = live && (unsigned)(x0 + col) < (unsigned)W;
#pragma unroll
        for (int r = 0; r < A; ++r) {
            const bool ok = cok && (unsigned)(y0 + r) < (unsigned)H;
            d[r] = ok ? *reinterpret_cast<const V*>(prow[r] + col * C) : V(0.f);
        }
        V o[A];
        bt_apply<S, FORM>(d, o);
#pragma unroll
        for (int i = 0; i < A; ++i) tt[i][col] = o[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Filter transform U = G g G^T of four input channels 4 kg .. 4 kg + 3 and output channel co, in double (off the hot path: once per
// weight update).  transposed = 0 reads a conv filter w_tf[R,R,Cin,Cout]; transposed = 1 a conv_transpose filter w_tf[R,R,Cout,Cin]
// with the taps flipped (a stride-1 transposed conv = the input gradient of the conv with that filter).  The FMAs are explicit: the
// fp32 pack and the split packs must round alike.  wino_filter_gg gathers the taps and leaves (G g)[i][q]; wino_filter_xi gives the
// four fp32 values of xi = (i, j).
template <class S>
__device__ __forceinline__ void wino_filter_gg(const float* w_tf, int Cin, int Cout, int kg, int co, int transposed,
                                               double (&gg)[S::TA][S::R][4])
{
    constexpr int A = S::TA, R = S::R;
    float g[R][R][4];
#pragma unroll
    for (int p_ = 0; p_ < R; ++p_)
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = kg * 4 + r;
                g[p_][q][r] = transposed ? w_tf[((size_t)((R - 1 - p_) * R + (R - 1 - q)) * Cout + co) * Cin + c]
                                         : w_tf[((size_t)(p_ * R + q) * Cin + c) * Cout + co];
            }
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double acc = 0.0;
#pragma unroll
                for (int p_ = 0; p_ < R; ++p_) acc = __builtin_fma(S::G(i, p_), (double)g[p_][q][r], acc);
                gg[i][q][r] = acc;
            }
}

template <class S>
__device__ __forceinline__ void wino_filter_xi(const double (&gg)[S::TA][S::R][4], int i, int j, float (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < S::R; ++q) acc = __builtin_fma(gg[i][q][r], S::G(j, q), acc);
        o[r] = (float)acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The operand split.  x -> three bf16 pieces, x = x0 + x1 + x2 exactly (v_cvt_pk_bf16_f32 rounds to nearest even; the remainders are
// exact in fp32).  split3_pair: two values at once -- one packed conversion per piece pair gives the word that is stored, its two halves
// widened again (a shift, a mask) feed one packed subtraction: 9 instructions per pair where split3<2> compiles to 15.
__device__ __forceinline__ void split3_pair(f32x2 x, unsigned (&w)[3])
{
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        w[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2));
        if (q < 2) {
            f32x2 h;
            h[0] = __builtin_bit_cast(float, w[q] << 16);
            h[1] = __builtin_bit_cast(float, w[q] & 0xffff0000u);
            x -= h;
        }
    }
}
__device__ __forceinline__ void split3_pair(float a, float b, unsigned (&w)[3]) { split3_pair(f32x2{a, b}, w); }

template <int VW>
__device__ __forceinline__ void split3(const float (&x)[VW], unsigned short (&p)[3][VW])
{
#pragma unroll
    for (int e = 0; e < VW; ++e) {
        const __bf16 h0 = (__bf16)x[e];
        const float r1 = x[e] - (float)h0;
        const __bf16 h1 = (__bf16)r1;
        const float r2 = r1 - (float)h1;
        const __bf16 h2 = (__bf16)r2;
        p[0][e] = __builtin_bit_cast(unsigned short, h0);
        p[1][e] = __builtin_bit_cast(unsigned short, h1);
        p[2][e] = __builtin_bit_cast(unsigned short, h2);
    }
}

// Format H2: two fp16 pieces of value / scale.  The scale is a power of two derived from max|x| of the UNtransformed tensor (a device
// word) times the factor by which the transform can grow a value (H2Bound: the squared largest absolute row sum of B^T, resp. G), so
// that every transformed value / scale is below 2^15: no overflow, and everything above 2^-18 of that keeps 22 mantissa bits.
__host__ __device__ inline float h2_scale(float amax, float bound)
{
    const float t = amax * bound * (1.0f / 32768.0f);
    if (!(t > 0.f)) return 1.f;                     // 0, and NaN (the max reduction drops NaNs; a NaN word itself lands here too)
    // max|x| = inf (an overflowed activation) or a product beyond the fp32 range: frexpf(inf) leaves the exponent unspecified.  The largest
    // power-of-two scale is used instead -- finite values then shrink towards 0, the inf itself stays inf in the fp16 piece and the output
    // is inf / NaN like the fp32 route's: deterministic, never an arbitrary scale.
    if (!(t <= 3.0e38f)) return 8.507059e37f;       // 2^126
    int e;
    const float m = frexpf(t, &e);                  // t = m * 2^e, 0.5 <= m < 1
    return ldexpf(1.f, m == 0.5f ? e - 1 : e);
}

template <class S> struct H2Bound {
    static constexpr float bt()
    {
        float m = 0.f;
        for (int i = 0; i < S::TA; ++i) { float r = 0.f; for (int k = 0; k < S::TA; ++k) r += S::BT(i, k) < 0.f ? -S::BT(i, k) : S::BT(i, k); m = r > m ? r : m; }
        return m * m;
    }
    static constexpr float g()
    {
        double m = 0.0;
        for (int i = 0; i < S::TA; ++i) { double r = 0.0; for (int k = 0; k < S::R; ++k) r += S::G(i, k) < 0.0 ? -S::G(i, k) : S::G(i, k); m = r > m ? r : m; }
        return (float)(m * m);
    }
};

// two scaled values -> the word of their first pieces (return) and of their second pieces (lo)
__device__ __forceinline__ unsigned h2_word(float a, float b, unsigned& lo)
{
    const _Float16 a0 = (_Float16)a, b0 = (_Float16)b;
    const _Float16 a1 = (_Float16)(a - (float)a0), b1 = (_Float16)(b - (float)b0);
    lo = (unsigned)__builtin_bit_cast(unsigned short, a1) | ((unsigned)__builtin_bit_cast(unsigned short, b1) << 16);
    return (unsigned)__builtin_bit_cast(unsigned short, a0) | ((unsigned)__builtin_bit_cast(unsigned short, b0) << 16);
}

// ---------------------------------------------------------------------------------------------------------------------
// Operand formats of the split GEMM stage.  A row of an operand panel holds, per K step of 16, NP planes of 16 values (32 bytes each).
//   B3: three bf16 pieces (exact sum = the fp32 value), six piece products i + j <= 2.  Rows of 96 bytes; the two 16-byte chunks
//       of a plane are swapped in rows with bit 3 set.
//   H2: the fp32 value divided by a power-of-two scale of its tensor, as two fp16 pieces (22-bit mantissa; values below 2^-18 of
//       the scaled maximum lose relative, not absolute, precision), three products (h0 h0, h0 h1, h1 h0); the accumulators are
//       multiplied by the two scales on the way out.  Rows of 64 bytes; the four chunks of a row are XORed with bits 2..3 of the
//       row index.  Either way the 16 lanes of a ds_read_b128 group (16 consecutive rows) hit 16 different bank groups.
// chunk(row, p, hb): byte offset inside a row of half hb (8 values) of plane p.  pair_words: two values of one row (already divided by
// the scale where SCALED) -> per plane the word that is stored.
// (a named namespace: profiler tables then show wino_gemm_bf3_kernel<rnf::FmtH2, 4, 2>)
namespace rnf {
struct FmtB3 {
    static constexpr int NP = 3, ROW = 96, NPROD = 6, ID = 0;
    static constexpr bool SCALED = false;
    typedef bf16x8 frag;
    static constexpr int PU[6] = {2, 1, 0, 1, 0, 0}, PV[6] = {0, 1, 2, 0, 1, 0};        // smallest terms first
    __device__ static __forceinline__ unsigned chunk(int row, int p, int hb) { return (unsigned)(p * 32) + ((((unsigned)hb) ^ (unsigned)((row >> 3) & 1)) << 4); }
    __device__ static __forceinline__ f32x16 mfma(const frag& u, const frag& v, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(u, v, c, 0, 0, 0); }
    __device__ static __forceinline__ void pair_words(float a, float b, unsigned (&w)[NP]) { split3_pair(a, b, w); }
};
struct FmtH2 {
    static constexpr int NP = 2, ROW = 64, NPROD = 3, ID = 1;
    static constexpr bool SCALED = true;
    typedef f16x8 frag;
    static constexpr int PU[6] = {1, 0, 0, 0, 0, 0}, PV[6] = {0, 1, 0, 0, 0, 0};
    __device__ static __forceinline__ unsigned chunk(int row, int p, int hb) { return (((unsigned)(p * 2 + hb)) ^ (unsigned)((row >> 2) & 3)) << 4; }
    __device__ static __forceinline__ f32x16 mfma(const frag& u, const frag& v, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(u, v, c, 0, 0, 0); }
    __device__ static __forceinline__ void pair_words(float a, float b, unsigned (&w)[NP]) { w[0] = h2_word(a, b, w[1]); }
};
}  // namespace rnf
