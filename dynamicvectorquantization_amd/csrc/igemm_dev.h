// Device pieces shared by the NT kernels (igemm_nt.hip), the TN kernels (igemm_tn.hip) and the fp32x3 plane kernels of the front end
// (igemm.hip: split8_bf16): tile constants, the LDS swizzles, the MFMA inner loops over one LDS stage, the fp32x3 operand split and the
// zero page.  Everything here has internal linkage: the build is not relocatable device code, so each of the three files carries its
// own copy (of g_zero_page: 32 bytes).
//
// Tile 128x128, 256 threads = 2x2 waves, each wave 2x2 MFMA 32x32 tiles (64 accumulator VGPRs).
// LDS rows are 128 B of K-contiguous data + 16 B pad (conflict-free ds_read_b128 for the MFMA
// fragment pattern), 2 stages x (A+B) = 72 KiB -> 2 workgroups per CU.  Global->LDS is register
// staged: loads for stage j+1 are issued before the MFMAs of stage j and written to LDS after them.
#pragma once
#include "dvq_common.h"

namespace igemm {
namespace {

constexpr int TILE = 128;
constexpr int ROWB = 144;                 // LDS bytes per tile row
constexpr int OPB = TILE * ROWB;          // one operand tile
constexpr int STAGEB = 2 * OPB;

template <typename T>
struct Vec {
    static constexpr int N = 16 / sizeof(T);   // elements per 16-B chunk
    static constexpr int BK = 128 / sizeof(T);  // K elements per stage
};

// -------------------------------------------------------------------------------------------------
// MFMA over one LDS stage: acc[mt][nt] += A(64 rows of this wave) x B(64 rows of this wave)^T
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void split8_bf16(const f32x4& c0, const f32x4& c1, bf16x8& hi, bf16x8& lo);

template <typename T>
__device__ __forceinline__ void mma_stage(const char* sA, const char* sB, f32x16 (&acc)[2][2], int wm, int wn,
                                          int lane, bool split3 = false) {     // (runtime flag: the register-staged kernel is an A/B path only)
    const int l31 = lane & 31, half = lane >> 5;
    const char* pa = sA + (wm * 64 + l31) * ROWB + half * 16;
    const char* pb = sB + (wn * 64 + l31) * ROWB + half * 16;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const bf16x8*>(pa + t * 32 * ROWB + ks * 32);
                b[t] = *reinterpret_cast<const bf16x8*>(pb + t * 32 * ROWB + ks * 32);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
    } else if (split3) {                     // fp32 operands as two bf16 planes, three MFMA passes (see split8_bf16)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                split8_bf16(*reinterpret_cast<const f32x4*>(pa + t * 32 * ROWB + (2 * u) * 32),
                            *reinterpret_cast<const f32x4*>(pa + t * 32 * ROWB + (2 * u + 1) * 32), ah[t], al[t]);
                split8_bf16(*reinterpret_cast<const f32x4*>(pb + t * 32 * ROWB + (2 * u) * 32),
                            *reinterpret_cast<const f32x4*>(pb + t * 32 * ROWB + (2 * u + 1) * 32), bh[t], bl[t]);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                }
        }
    } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const f32x4*>(pa + t * 32 * ROWB + jj * 32);
                b[t] = *reinterpret_cast<const f32x4*>(pb + t * 32 * ROWB + jj * 32);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][s], b[nt][s], acc[mt][nt], 0, 0, 0);
        }
    }
}

// 16-byte zero page of the LDS-DMA kernels: out-of-image taps and K / row tails read it instead of being predicated
__device__ uint4 g_zero_page[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};

constexpr int GROW = 128;               // unpadded LDS row bytes
constexpr int GOPB = TILE * GROW;       // 16 KiB per operand tile
constexpr int GSTAGEB = 2 * GOPB;

// swizzle kinds for unpadded 128-B LDS rows: chunk c of row r is stored at chunk position c ^ f(r)
//   SWZ_NT: f(r) = (r >> 1) & 7                                   (conflict-free b128 fragment reads; DMA fill)
//   SWZ_TN: f(r) = ((r >> 3) & 3) | (((r >> 1) ^ (r >> 5)) & 1) << 2
//           additionally conflict-free for the transposing stores of the TN loader, where 8 consecutive lanes
//           write rows 8 apart (found by exhaustive search over XOR-linear maps)
enum { SWZ_NT = 0, SWZ_TN = 1 };
__device__ __forceinline__ int swz_tn(int r) { return ((r >> 3) & 3) | ((((r >> 1) ^ (r >> 5)) & 1) << 2); }

// fp32 operands on the bf16 matrix pipe (dvq_set_fp32_split, round 5): x = hi + lo with hi = x rounded to bf16 and lo = x - hi (exact in
// fp32, |lo| <= 2^-9 |x|) rounded to bf16; the product runs as lo.hi + hi.lo + hi.hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation --
// the VQ search's scheme (section 4) -- ~2^-17 relative error per term (lo.lo dropped, lo rounded) instead of 2^-24, at 3/16 of the
// fp32-MFMA issue time.  The lane's 8
// k-values of a 16-k step are the two 4-float chunks it would feed to v_mfma_f32_32x32x2_f32 one by one: A and B use the same chunk
// arithmetic, so element e of lane (row, half) is the same k on both sides -- any such pairing is a valid contraction order.
__device__ __forceinline__ void split8_bf16(const f32x4& c0, const f32x4& c1, bf16x8& hi, bf16x8& lo) {
    dvq_u32x4 h, l;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const f32x4& c = q == 0 ? c0 : c1;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const unsigned ph = pack_bf16x2(c[2 * e], c[2 * e + 1]);                     // round to nearest even
            h[2 * q + e] = ph;
            const float r0 = c[2 * e] - __uint_as_float(ph << 16), r1 = c[2 * e + 1] - __uint_as_float(ph & 0xffff0000u);
            l[2 * q + e] = pack_bf16x2(r0, r1);
        }
    }
    hi = __builtin_bit_cast(bf16x8, h);
    lo = __builtin_bit_cast(bf16x8, l);
}

template <typename T, int SWZ = SWZ_NT, bool S3 = false>
__device__ __forceinline__ void mma_stage_swz(const char* sA, const char* sB, f32x16 (&acc)[2][2], int wm, int wn,
                                              int lane) {
    const int l31 = lane & 31, half = lane >> 5;
    // rows are wm*64 + t*32 + l31: only bit 5 of the row depends on t
    int swz[2];
    swz[0] = SWZ == SWZ_NT ? ((l31 >> 1) & 7) : swz_tn(l31);
    swz[1] = SWZ == SWZ_NT ? swz[0] : swz_tn(l31 + 32);
    const char* pa = sA + (wm * 64 + l31) * GROW;
    const char* pb = sB + (wn * 64 + l31) * GROW;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int off = ((ks * 2 + half) ^ swz[t]) << 4;
                a[t] = *reinterpret_cast<const bf16x8*>(pa + t * 32 * GROW + off);
                b[t] = *reinterpret_cast<const bf16x8*>(pb + t * 32 * GROW + off);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
    } else if constexpr (S3) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int o0 = ((4 * u + half) ^ swz[t]) << 4, o1 = ((4 * u + 2 + half) ^ swz[t]) << 4;
                split8_bf16(*reinterpret_cast<const f32x4*>(pa + t * 32 * GROW + o0), *reinterpret_cast<const f32x4*>(pa + t * 32 * GROW + o1),
                            ah[t], al[t]);
                split8_bf16(*reinterpret_cast<const f32x4*>(pb + t * 32 * GROW + o0), *reinterpret_cast<const f32x4*>(pb + t * 32 * GROW + o1),
                            bh[t], bl[t]);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                }
        }
    } else {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int off = ((jj * 2 + half) ^ swz[t]) << 4;
                a[t] = *reinterpret_cast<const f32x4*>(pa + t * 32 * GROW + off);
                b[t] = *reinterpret_cast<const f32x4*>(pb + t * 32 * GROW + off);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][s], b[nt][s], acc[mt][nt], 0, 0, 0);
        }
    }
}

constexpr int WT = 256;                       // macro tile (rows and columns)
constexpr int WOPB = WT * GROW;               // 32 KiB per operand slab
constexpr int WSTAGEB = 2 * WOPB;             // 64 KiB per stage

typedef int int32x4 __attribute__((ext_vector_type(4)));      // buffer resource descriptor (SGPR quadruple)

}  // namespace
}  // namespace igemm
