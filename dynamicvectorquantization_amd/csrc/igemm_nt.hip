// NT side of the implicit-GEMM convolution / batched GEMM (map of the files: igemm.hip):
//   C[m][n] = sum_k A[m][k] * B[n][k]      A rows are gathered on the fly (im2col never exists)
// Kernels (register-staged, LDS-DMA, wide, wide-pipe, 8-phase, conv-pipe, skinny, naive), epilogues, predicates, launchers and launch_nt.
#include <type_traits>

#include "igemm.h"
#include "igemm_dev.h"

namespace igemm {
namespace {

// parity-class row order of the stride-2 input gradient: class-local index m -> (image, y, x) of class pc = 2 * (y & 1) + (x & 1)
__device__ __forceinline__ int64_t par_out_row(const NtParams& p, int pc, int m) {
    const int hw2 = (p.DH >> 1) * (p.DW >> 1), w2 = p.DW >> 1;
    const int n = m / hw2, rem = m - n * hw2;
    const int yy = rem / w2, xx = rem - yy * w2;
    return ((int64_t)n * p.DH + 2 * yy + (pc >> 1)) * p.DW + 2 * xx + (pc & 1);
}

// -------------------------------------------------------------------------------------------------
// NT epilogue: alpha * acc + bias (+ residual) -> C, shared by the register-staged and the LDS-DMA kernels
// -------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void nt_epilogue(const NtParams& p, f32x16 (&acc)[2][2], int m0, int n0, int64_t bz, int wm,
                                            int wn, int lane) {
    T* __restrict__ Cg = reinterpret_cast<T*>(p.C) + bz * p.sC;
    const T* __restrict__ Rg = p.R ? reinterpret_cast<const T*>(p.R) + bz * p.sC : nullptr;
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int col = n0 + wn * 64 + nt * 32 + l31;
        if (col >= p.Ncols) continue;
        const float bcol = p.bias_mode == 1 ? p.bias[col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < p.M) {
                    float v = acc[mt][nt][r] * p.alpha + bcol;
                    if (p.bias_mode == 2) v += p.bias[row];
                    const int64_t o = (int64_t)row * p.ldc + col;
                    if (Rg) {
                        const float rr = ElemIO<T>::load(Rg + o);
                        if (p.res_mask) v *= rr > 0.f ? 1.f : p.mask_slope;
                        else v += rr;
                    }
                    v = v > 0.f ? v : v * p.act_slope;
                    ElemIO<T>::store(Cg + o, v);
                }
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Vectorised NT epilogue: the 128x128 tile goes through LDS (as T) so that global stores and the residual
// read are full 16-byte accesses along the channel dimension instead of 2-byte scalar accesses.
// Caller guarantees a preceding __syncthreads() (all MFMA reads of smem are done) and ldc % VN == 0.
// -------------------------------------------------------------------------------------------------
// residual handling of the vectorised epilogue: add (then activation) or gate
__device__ __forceinline__ float nt_res(const NtParams& p, float v, float r) {
    if (p.res_mask) return v * (r > 0.f ? 1.f : p.mask_slope);
    v += r;
    return v > 0.f ? v : v * p.act_slope;
}

template <typename T>
__device__ __forceinline__ void nt_epilogue_vec(const NtParams& p, f32x16 (&acc)[2][2], char* smem, int m0, int n0,
                                                int64_t bz, int wm, int wn, int tid, int pc = -1) {
    constexpr int VN = Vec<T>::N;
    constexpr int ROW = TILE * (int)sizeof(T);          // staged row bytes (256 / 512)
    const int lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    T* st = reinterpret_cast<T*>(smem);
    const bool early_act = p.R == nullptr || p.res_mask;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int lc = wn * 64 + nt * 32 + l31;
        const int col = n0 + lc;
        const float bcol = (p.bias_mode == 1 && col < p.Ncols) ? p.bias[col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                float v = acc[mt][nt][r] * p.alpha + bcol;
                if (p.bias_mode == 2 && m0 + lr < p.M) v += p.bias[m0 + lr];
                if (early_act) v = v > 0.f ? v : v * p.act_slope;
                ElemIO<T>::store(st + lr * TILE + lc, v);
            }
    }
    __syncthreads();
    T* __restrict__ Cg = reinterpret_cast<T*>(p.C) + bz * p.sC;
    const T* __restrict__ Rg = p.R ? reinterpret_cast<const T*>(p.R) + bz * p.sC : nullptr;
    constexpr int CPR = TILE / VN;                       // 16-byte chunks per staged row
#pragma unroll
    for (int i = 0; i < (TILE * CPR) / 256; ++i) {
        const int q = tid + 256 * i;
        const int lr = q / CPR, ch = q % CPR;
        const int row = m0 + lr, col = n0 + ch * VN;
        if (row >= (pc < 0 ? p.M : p.M >> 2) || col >= p.Ncols) continue;
        uint4 v = *reinterpret_cast<const uint4*>(smem + lr * ROW + ch * 16);
        const int64_t o = (pc < 0 ? (int64_t)row : par_out_row(p, pc, row)) * p.ldc + col;
        if (col + VN <= p.Ncols) {
            if (Rg) {
                const uint4 rv = *reinterpret_cast<const uint4*>(Rg + o);
                if constexpr (sizeof(T) == 2) {
                    unsigned* pv = &v.x;
                    const unsigned* pr = &rv.x;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float lo = nt_res(p, __uint_as_float(pv[k] << 16), __uint_as_float(pr[k] << 16));
                        const float hi = nt_res(p, __uint_as_float(pv[k] & 0xffff0000u), __uint_as_float(pr[k] & 0xffff0000u));
                        pv[k] = pack_bf16x2(lo, hi);
                    }
                } else {
                    float* pv = reinterpret_cast<float*>(&v.x);
                    const float* pr = reinterpret_cast<const float*>(&rv.x);
#pragma unroll
                    for (int k = 0; k < 4; ++k) pv[k] = nt_res(p, pv[k], pr[k]);
                }
            }
            *reinterpret_cast<uint4*>(Cg + o) = v;
        } else {      // ragged last chunk of a row (Ncols % VN != 0): element-wise
            const T* sv = reinterpret_cast<const T*>(&v);
            for (int k = 0; k < VN && col + k < p.Ncols; ++k) {
                float f = ElemIO<T>::load(sv + k);
                if (Rg) f = nt_res(p, f, ElemIO<T>::load(Rg + o + k));
                ElemIO<T>::store(Cg + o + k, f);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// NT kernel
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void igemm_nt_kernel(NtParams p) {
    constexpr int VN = Vec<T>::N;
    constexpr int BK = Vec<T>::BK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int wi = xcd_remap(blockIdx.x, p.gm * p.gn);
    const int m0 = (wi / p.gn) * TILE, n0 = (wi % p.gn) * TILE;
    const int64_t bz = blockIdx.z;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;

    const int ch = tid & 7;         // 16-B chunk within the 128-B row
    const int r0 = tid >> 3;        // rows r0 + 32*i
    // per-row gather state
    int rn[4], ra[4], rb[4];
    bool rok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + r0 + 32 * i;
        rok[i] = m < p.M;
        const int mm = rok[i] ? m : 0;
        if (p.mode == MODE_GEMM) {
            rn[i] = mm;
            ra[i] = rb[i] = 0;
        } else {
            const int hw = p.DH * p.DW;
            const int n = mm / hw, rem = mm - n * hw;
            const int y = rem / p.DW, x = rem - y * p.DW;
            rn[i] = n;
            if (p.mode == MODE_FWD) {
                ra[i] = y * p.stride - p.pad_t;
                rb[i] = x * p.stride - p.pad_l;
            } else {
                ra[i] = y + p.pad_t;
                rb[i] = x + p.pad_l;
            }
        }
    }
    const int cpt = (int)(p.lda / VN);   // conv: 16-B units per tap
    const int sshift = p.stride == 2 ? 1 : 0;
    // B rows
    int64_t boff[4];
    bool bok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + r0 + 32 * i;
        bok[i] = n < p.Ncols;
        boff[i] = (int64_t)(bok[i] ? n : 0) * p.ldb;
    }

    uint4 pa[4], pb[4];
    auto g_load = [&](int j) {
        const int u = j * 8 + ch;              // 16-B unit index along K
        const int ke = u * VN;
        const bool kok = ke < p.Ktot;
        int kh = 0, kw = 0, c0 = ke;
        if (p.mode != MODE_GEMM) {
            const int tap = u / cpt;
            c0 = (u - tap * cpt) * VN;
            kh = tap / p.KW;
            kw = tap - kh * p.KW;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool ok = kok && rok[i];
            int64_t off = 0;
            if (p.mode == MODE_GEMM) {
                off = (int64_t)rn[i] * p.lda + ke;
            } else if (p.mode == MODE_FWD) {
                const int ih = ra[i] + kh, iw = rb[i] + kw;
                ok = ok && (unsigned)ih < (unsigned)p.LH && (unsigned)iw < (unsigned)p.LW;
                off = (((int64_t)rn[i] * p.SH + (ih >> p.up)) * p.SW + (iw >> p.up)) * p.lda + c0;
            } else {
                const int t = ra[i] - kh, v = rb[i] - kw;
                const int mask = p.stride - 1;
                ok = ok && t >= 0 && v >= 0 && ((t | v) & mask) == 0;
                const int oh = t >> sshift, ow = v >> sshift;
                ok = ok && oh < p.LH && ow < p.LW;
                off = (((int64_t)rn[i] * p.SH + oh) * p.SW + ow) * p.lda + c0;
            }
            pa[i] = ok ? *reinterpret_cast<const uint4*>(Ag + off) : make_uint4(0, 0, 0, 0);
            pb[i] = (kok && bok[i]) ? *reinterpret_cast<const uint4*>(Bg + boff[i] + ke) : make_uint4(0, 0, 0, 0);
        }
    };
    auto s_store = [&](int buf) {
        char* sa = smem + buf * STAGEB + r0 * ROWB + ch * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<uint4*>(sa + i * 32 * ROWB) = pa[i];
            *reinterpret_cast<uint4*>(sa + OPB + i * 32 * ROWB) = pb[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = (p.Ktot + BK - 1) / BK;
    g_load(0);
    s_store(0);
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
        const int buf = j & 1;
        if (j + 1 < nk) g_load(j + 1);
        mma_stage<T>(smem + buf * STAGEB, smem + buf * STAGEB + OPB, acc, wm, wn, lane, p.split3 != 0);
        if (j + 1 < nk) s_store(buf ^ 1);
        __syncthreads();
    }

    nt_epilogue<T>(p, acc, m0, n0, bz, wm, wn, lane);
}

// -------------------------------------------------------------------------------------------------
// NT kernel, LDS-DMA staging (global_load_lds_dwordx4): no VGPR round trip, no ds_write.
// LDS tile rows are 128 B unpadded; the 16-B chunk c of row r lives at chunk position c ^ ((r >> 1) & 7)
// (the DMA writes lane-linear, so the permutation is applied to the per-lane SOURCE address and again on
// the fragment read: conflict-free ds_read_b128 for the MFMA pattern).  Out-of-image taps and K / row
// tails read a 16-byte zero page instead of being predicated.
// -------------------------------------------------------------------------------------------------
template <typename T, int MODE, bool TAPU, bool S3 = false>      // S3: fp32 operands as two bf16 planes, three bf16 MFMA passes (fp32x3)
__global__ __launch_bounds__(256, 2) void igemm_nt_glds_kernel(NtParams p) {
    constexpr int VN = Vec<T>::N;
    constexpr int BK = Vec<T>::BK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int wi = xcd_remap(blockIdx.x, p.gm * p.gn);
    int mtile = wi / p.gn;
    const int n0 = (wi % p.gn) * TILE;
    // stride-2 input gradient by parity class (p.par): tiles [pc * par_tiles, (pc + 1) * par_tiles) hold the pixels of class pc
    const bool par = MODE == MODE_TCONV && TAPU && p.par != 0;
    int pc = -1, Mrows = p.M, khc = 0, kwc = 0, nkw = 1, Kcls = p.Ktot;
    if (par) {
        pc = mtile / p.par_tiles;
        mtile -= pc * p.par_tiles;
        Mrows = p.M >> 2;
        khc = ((pc >> 1) + p.pad_t) & 1;
        kwc = ((pc & 1) + p.pad_l) & 1;
        const int khn = p.Ktot / (int)p.lda / p.KW;              // KH
        const int nkh = (khn - khc + 1) >> 1;
        nkw = (p.KW - kwc + 1) >> 1;
        Kcls = nkh * nkw * (int)p.lda;
    }
    const int m0 = mtile * TILE;
    const int64_t bz = blockIdx.z;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const T* zero = reinterpret_cast<const T*>(g_zero_page);

    // DMA instruction i of this wave fills tile rows wave*32 + i*8 .. +7 (one 1-KiB piece); lane -> (row, chunk pos)
    const int lrow = lane >> 3, cpos = lane & 7;
    int rn[4], ra[4], rb[4], cg[4];
    bool rok[4];
    int64_t boff[4];
    bool bok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int trow = wave * 32 + i * 8 + lrow;
        cg[i] = cpos ^ ((trow >> 1) & 7);          // which 16-B chunk of the row this lane fetches
        const int m = m0 + trow;
        rok[i] = m < Mrows;
        const int mm = rok[i] ? m : 0;
        if constexpr (MODE == MODE_GEMM) {
            rn[i] = mm;
            ra[i] = rb[i] = 0;
        } else {
            const int dw_ = par ? p.DW >> 1 : p.DW;
            const int hw = par ? (p.DH >> 1) * dw_ : p.DH * p.DW;
            const int n = mm / hw, rem = mm - n * hw;
            int y = rem / dw_, x = rem - y * dw_;
            if (par) {
                y = 2 * y + (pc >> 1);
                x = 2 * x + (pc & 1);
            }
            rn[i] = n * p.SH * p.SW;                // source pixel base of image n
            if constexpr (MODE == MODE_FWD) {
                ra[i] = y * p.stride - p.pad_t;
                rb[i] = x * p.stride - p.pad_l;
            } else {
                ra[i] = y + p.pad_t;
                rb[i] = x + p.pad_l;
            }
        }
        const int nn = n0 + trow;
        bok[i] = nn < p.Ncols;
        boff[i] = (int64_t)(bok[i] ? nn : 0) * p.ldb;
    }
    const int cpt = (int)(p.lda / VN);              // conv: 16-B units per tap
    constexpr bool tap_uniform = TAPU;              // a K stage never straddles a tap ((Cs / VN) % 8 == 0)
    const int sshift = p.stride == 2 ? 1 : 0;
    const int smask = p.stride - 1;

    auto issue = [&](int j, int buf) {
        char* sa = smem + buf * GSTAGEB + wave * 32 * GROW;
        int kh0 = 0, kw0 = 0, cu0 = 0;
        if constexpr (MODE != MODE_GEMM && tap_uniform) {
            const int tap = (j * 8) / cpt;
            cu0 = j * 8 - tap * cpt;
            if (par) {                                   // tap-th VALID tap of this parity class
                const int a = tap / nkw;
                kh0 = khc + 2 * a;
                kw0 = kwc + 2 * (tap - a * nkw);
            } else {
                kh0 = tap / p.KW;
                kw0 = tap - kh0 * p.KW;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = j * 8 + cg[i];
            int ke = u * VN;
            const bool kok = ke < Kcls;
            bool ok = kok && rok[i];
            int64_t off = 0;
            if constexpr (MODE == MODE_GEMM) {
                off = (int64_t)rn[i] * p.lda + ke;
            } else {
                int kh = kh0, kw = kw0, c0 = (cu0 + cg[i]) * VN;
                if constexpr (!tap_uniform) {
                    const int tap = u / cpt;
                    c0 = (u - tap * cpt) * VN;
                    kh = tap / p.KW;
                    kw = tap - kh * p.KW;
                }
                if constexpr (MODE == MODE_FWD) {
                    const int ih = ra[i] + kh, iw = rb[i] + kw;
                    ok = ok && (unsigned)ih < (unsigned)p.LH && (unsigned)iw < (unsigned)p.LW;
                    off = (int64_t)(rn[i] + (ih >> p.up) * p.SW + (iw >> p.up)) * p.lda + c0;
                } else {
                    const int t = ra[i] - kh, v = rb[i] - kw;
                    ok = ok && t >= 0 && v >= 0 && ((t | v) & smask) == 0;
                    const int oh = t >> sshift, ow = v >> sshift;
                    ok = ok && oh < p.LH && ow < p.LW;
                    off = (int64_t)(rn[i] + oh * p.SW + ow) * p.lda + c0;
                    if (par) ke = (kh * p.KW + kw) * (int)p.lda + c0;      // weight columns of the real tap
                }
            }
            const T* srcA = ok ? Ag + off : zero;
            const T* srcB = (kok && bok[i]) ? Bg + boff[i] + ke : zero;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcA,
                                             (__attribute__((address_space(3))) void*)(sa + i * 8 * GROW), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcB,
                                             (__attribute__((address_space(3))) void*)(sa + GOPB + i * 8 * GROW), 16, 0, 0);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = (Kcls + BK - 1) / BK;
    issue(0, 0);
    dvq_dma_barrier();                 // drains the DMA (vmcnt(0)) and publishes the stage
    for (int j = 0; j < nk; ++j) {
        const int buf = j & 1;
        if (j + 1 < nk) issue(j + 1, buf ^ 1);
        mma_stage_swz<T, SWZ_NT, S3>(smem + buf * GSTAGEB, smem + buf * GSTAGEB + GOPB, acc, wm, wn, lane);
        dvq_dma_barrier();
    }
    if ((p.ldc % VN) == 0) {
        nt_epilogue_vec<T>(p, acc, smem, m0, n0, bz, wm, wn, tid, pc);     // LDS-staged, 16-byte global accesses
    } else {
        nt_epilogue<T>(p, acc, m0, n0, bz, wm, wn, lane);
    }
}

// -------------------------------------------------------------------------------------------------
// Wide NT GEMM (bf16): 256 x 256 macro tile, 8 waves x (2 x 4) 32x32x16 MFMA tiles, 64-element K slabs double-buffered through
// LDS-DMA (2 x 64 KiB), one workgroup per CU.  Six fragment reads feed eight MFMAs (the 128 x 128 kernel above needs four
// per four) and every operand byte fetched from L2 feeds twice as many flops: used for the large plain GEMMs (StackGPT
// linears and their input gradients, attention score products).  Same swizzle / zero-page conventions as above.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void gemm_nt_wide_kernel(NtParams p) {
    using T = bf16_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                 // 4 x 2 waves: 64 rows x 128 columns each
    const int l31 = lane & 31, half = lane >> 5;
    const int wi = xcd_remap(blockIdx.x, p.gm * p.gn);
    const int m0 = (wi / p.gn) * WT, n0 = (wi % p.gn) * WT;
    const int64_t bz = blockIdx.z;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const T* zero = reinterpret_cast<const T*>(g_zero_page);
    const int lrow = lane >> 3, cpos = lane & 7;
    int64_t aoff[4], boff[4];
    bool aok[4], bok[4];
    int cg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int trow = wave * 32 + i * 8 + lrow;
        cg[i] = cpos ^ ((trow >> 1) & 7);
        aok[i] = m0 + trow < p.M;
        bok[i] = n0 + trow < p.Ncols;
        aoff[i] = (int64_t)(aok[i] ? m0 + trow : 0) * p.lda;
        boff[i] = (int64_t)(bok[i] ? n0 + trow : 0) * p.ldb;
    }
    auto issue = [&](int j, int buf) {
        char* sa = smem + buf * WSTAGEB + wave * 32 * GROW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ke = (j * 8 + cg[i]) * 8;
            const bool kok = ke < p.Ktot;
            const T* srcA = (kok && aok[i]) ? Ag + aoff[i] + ke : zero;
            const T* srcB = (kok && bok[i]) ? Bg + boff[i] + ke : zero;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcA,
                                             (__attribute__((address_space(3))) void*)(sa + i * 8 * GROW), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcB,
                                             (__attribute__((address_space(3))) void*)(sa + WOPB + i * 8 * GROW), 16, 0, 0);
        }
    };
    f32x16 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int swz = (l31 >> 1) & 7;                           // rows differ from l31 by multiples of 32: same swizzle
    const int nk = (p.Ktot + 63) / 64;
    issue(0, 0);
    dvq_dma_barrier();
    for (int j = 0; j < nk; ++j) {
        const int buf = j & 1;
        if (j + 1 < nk) issue(j + 1, buf ^ 1);
        const char* pa = smem + buf * WSTAGEB + (wm * 64 + l31) * GROW;
        const char* pb = smem + buf * WSTAGEB + WOPB + (wn * 128 + l31) * GROW;
        bf16x8 a[2][2], b[2][4];
        auto load_frags = [&](int ks, int slot) {
            const int off = ((ks * 2 + half) ^ swz) << 4;
#pragma unroll
            for (int t = 0; t < 2; ++t) a[slot][t] = *reinterpret_cast<const bf16x8*>(pa + t * 32 * GROW + off);
#pragma unroll
            for (int t = 0; t < 4; ++t) b[slot][t] = *reinterpret_cast<const bf16x8*>(pb + t * 32 * GROW + off);
        };
        load_frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + 1 < 4) load_frags(ks + 1, (ks + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks & 1][mt], b[ks & 1][nt], acc[mt][nt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        dvq_dma_barrier();
    }
    // epilogue: the 256 x 256 tile is staged as bf16 (128 KiB = both stages) and leaves in 16-byte stores
    T* st = reinterpret_cast<T*>(smem);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int lc = wn * 128 + nt * 32 + l31;
        const float bcol = (p.bias_mode == 1 && n0 + lc < p.Ncols) ? p.bias[n0 + lc] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                float v = acc[mt][nt][r] * p.alpha + bcol;
                if (p.bias_mode == 2 && m0 + lr < p.M) v += p.bias[m0 + lr];
                v = v > 0.f ? v : v * p.act_slope;
                st[lr * WT + lc] = f32_to_bf16(v);
            }
    }
    __syncthreads();
    T* __restrict__ Cg = reinterpret_cast<T*>(p.C) + bz * p.sC;
#pragma unroll 4
    for (int i = 0; i < (WT * WT / 8) / 512; ++i) {
        const int q = tid + 512 * i;
        const int lr = q >> 5, ch = q & 31;
        const int row = m0 + lr, col = n0 + ch * 8;
        if (row >= p.M || col >= p.Ncols) continue;
        const uint4 v = *reinterpret_cast<const uint4*>(smem + lr * (WT * 2) + ch * 16);
        T* dst = Cg + (int64_t)row * p.ldc + col;
        if (col + 8 <= p.Ncols) {
            *reinterpret_cast<uint4*>(dst) = v;
        } else {
            const T* sv = reinterpret_cast<const T*>(&v);
            for (int k = 0; k < 8 && col + k < p.Ncols; ++k) dst[k] = sv[k];
        }
    }
}

// -------------------------------------------------------------------------------------------------
// The same 256 x 256 NT GEMM with the main loop pipelined like conv_halo.hip's: per 16-k step the 8 MFMAs of a wave are issued
// with the next step's 6 fragment reads and (in the first two steps of a K slab) the next slab's 8 DMA pieces slotted between
// them (sched_group_barrier); the slab barrier sits before the LAST step, whose MFMAs cover the first fragment reads of the next
// slab.  The MFMAs compute (B A^T), so a lane ends up with 4 CONSECUTIVE output columns of one row per register quad: the tile
// is staged with packed 8-byte LDS stores (64 per lane instead of 128 2-byte ones; 16-byte chunk c of row r at c ^ (r & 31)).
// Rows past M / Ncols re-read the last real row (never stored) instead of a zero page.  Needs Ncols % 8 == 0, Ktot % 64 == 0.
// -------------------------------------------------------------------------------------------------
// WMW x WNW waves of MT x (8 / WNW) MFMA tiles each:
//   4 x 2 x (2 x 4): 256-row tile, two waves per SIMD (the default);
//   2 x 2 x (4 x 4): 256-row tile, 256 accumulator registers, ONE wave per SIMD -- 8 fragment reads feed 16 MFMAs instead of 6
//                    feeding 8; measured no faster;
//   2 x 2 x (3 x 4): 192-row tile for shapes whose 256-row tiling fills the last round badly: 20736 tokens x 1024 columns are 324
//                    tiles of 256 rows -- two rounds on 256 CUs, the second a quarter full -- but 432 of 192 rows: two rounds of
//                    0.75.  (Six waves of 2 x 4 tiles would load the four SIMDs 2 : 2 : 1 : 1.)
template <int WMW, int WNW, int MT>
__global__ __launch_bounds__(64 * WMW * WNW, WMW * WNW == 4 ? 1 : 2) void gemm_nt_wide_pipe_kernel(NtParams p) {
#if defined(__HIP_DEVICE_COMPILE__)      // (buffer-descriptor builtins exist in the device pass only; the host pass needs just the stub)
    using T = bf16_t;
    constexpr int NWV = WMW * WNW, NTH = 64 * NWV;
    constexpr int NT = WT / 32 / WNW;                        // MFMA tiles per wave: MT x NT
    constexpr int TM = WMW * MT * 32;                        // tile rows (256 or 192); tile columns: WT = 256
    constexpr int NM = MT * NT, DS = MT + NT;                // MFMAs / fragment reads per 16-k step
    constexpr int NPA = TM / 8 / NWV;                        // DMA pieces (8 rows) per wave and K slab: A
    constexpr int NPB = (WT / 8 + NWV - 1) / NWV;            //   and B (6 waves: 36 for 32 pieces, the last one sent repeatedly)
    constexpr int AOPB = TM * GROW;                          // bytes of an A slab; a stage = A slab + B slab
    constexpr int STG = AOPB + WOPB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WNW, wn = wave % WNW;
    const int l31 = lane & 31, half = lane >> 5;
    // tile order: the 32 workgroups an XCD runs at a time (consecutive indices after xcd_remap) cover a block of 8 tile rows x 4
    // tile columns -- 12 operand slabs per K step through that XCD's L2 instead of the 33 of a row-major strip
    const int wi = xcd_remap(blockIdx.x, p.gm * p.gn);
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * p.gn;
    const int grp = wi / per_group, rem = wi - grp * per_group;
    const int gsz = min(p.gm - grp * GROUP_M, GROUP_M);
    const int m0 = (grp * GROUP_M + rem % gsz) * TM, n0 = (rem / gsz) * WT;
    const int64_t bz = blockIdx.z;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const int lrow = lane >> 3, cpos = lane & 7;
    // DMA through buffer descriptors: the operand base lives in SGPRs, a lane contributes one 32-bit byte offset (fixed for the
    // whole kernel) and the K slab is the scalar offset -- no per-piece address arithmetic and half the address traffic of
    // global_load_lds with 64-bit lane addresses.  (Launcher: Ktot % 64 == 0, operands below 2 GiB.)
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(Ag), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(Bg), 0, 0x7fffffff, 0x00020000);
    int aoff[NPA], boff[NPB];
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        const int trow = (wave * NPA + i) * 8 + lrow;
        aoff[i] = (int)(((int64_t)min(m0 + trow, p.M - 1) * p.lda + (cpos ^ ((trow >> 1) & 7)) * 8) * 2);
    }
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
        const int trow = min(wave * NPB + i, WT / 8 - 1) * 8 + lrow;
        boff[i] = (int)(((int64_t)min(n0 + trow, p.Ncols - 1) * p.ldb + (cpos ^ ((trow >> 1) & 7)) * 8) * 2);
    }
    constexpr int ND = NPA + NPB;
    auto issue_one = [&](int q, int j, int buf) {            // DMA instruction q of K slab j: A piece q, or B piece q - NPA
        if (q < NPA)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsA, (__attribute__((address_space(3))) void*)(smem + buf * STG + (wave * NPA + q) * 8 * GROW), 16, aoff[q], j * 128, 0, 0);
        else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsB, (__attribute__((address_space(3))) void*)(smem + buf * STG + AOPB + min(wave * NPB + q - NPA, WT / 8 - 1) * 8 * GROW),
                16, boff[q - NPA], j * 128, 0, 0);
    };
    f32x16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int swz = (l31 >> 1) & 7;                           // rows differ from l31 by multiples of 32: same swizzle
    const int nk = (p.Ktot + 63) / 64;
    const char* pa;
    const char* pb;
    auto set_stage = [&](int buf) {
        pa = smem + buf * STG + (wm * (MT * 32) + l31) * GROW;
        pb = smem + buf * STG + AOPB + (wn * (NT * 32) + l31) * GROW;
    };
    bf16x8 a[2][MT], b[2][NT];
    auto load_frags = [&](int ks, int slot) {                 // in the order the MFMAs consume them
        const int off = ((ks * 2 + half) ^ swz) << 4;
        a[slot][0] = *reinterpret_cast<const bf16x8*>(pa + off);
#pragma unroll
        for (int t = 0; t < NT; ++t) b[slot][t] = *reinterpret_cast<const bf16x8*>(pb + t * 32 * GROW + off);
#pragma unroll
        for (int t = 1; t < MT; ++t) a[slot][t] = *reinterpret_cast<const bf16x8*>(pa + t * 32 * GROW + off);
    };
    // the MFMAs of a step and the issue order around them: the fragment reads of the next step two by two right behind the first
    // MFMAs (they have landed long before the next step starts), then one DMA instruction behind each following MFMA
    auto mfma_step = [&](int slot, auto vm_tag) {
        constexpr int VM = decltype(vm_tag)::value;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[slot][nt], a[slot][mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (2 * i < DS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            else if (i - DS / 2 < VM) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // The DMA instructions of K slab j + 1 are spread over THREE steps -- the last step of slab j - 1 (the stage is free from
    // that slab's barrier on), and the first two of slab j -- so that the texture-address path sees ~3 KiB per wave and step instead
    // of bursts of 4 KiB, and two more steps of MFMAs lie between the last DMA and the barrier that waits for it.
    constexpr int Q0 = (ND + 2) / 3, Q1 = Q0 + (ND - Q0 + 1) / 2;     // [0, Q0) | [Q0, Q1) | [Q1, ND)
    using V0 = std::integral_constant<int, 0>;
    using VA = std::integral_constant<int, Q0>;
    using VB = std::integral_constant<int, Q1 - Q0>;
    using VC = std::integral_constant<int, ND - Q1>;
#pragma unroll
    for (int q = 0; q < ND; ++q) issue_one(q, 0, 0);
    dvq_dma_barrier();
    set_stage(0);
    load_frags(0, 0);
#pragma unroll
    for (int q = 0; q < Q0; ++q) issue_one(q, nk > 1 ? 1 : 0, 1);
#pragma unroll 1
    for (int j = 0; j < nk; ++j) {
        const int buf = j & 1;
        const int jn = j + 1 < nk ? j + 1 : nk - 1;           // (past the end: harmless re-fetches into dead stages)
        const int jnn = j + 2 < nk ? j + 2 : nk - 1;
        __builtin_amdgcn_sched_barrier(0);
        load_frags(1, 1);
#pragma unroll
        for (int q = Q0; q < Q1; ++q) issue_one(q, jn, buf ^ 1);
        mfma_step(0, VB{});
        load_frags(2, 0);
#pragma unroll
        for (int q = Q1; q < ND; ++q) issue_one(q, jn, buf ^ 1);
        mfma_step(1, VC{});
        load_frags(3, 1);
        mfma_step(0, V0{});
        dvq_dma_barrier();          // every wave has its reads of this slab behind it and its pieces of the next one landed
        set_stage(buf ^ 1);
        load_frags(0, 0);
#pragma unroll
        for (int q = 0; q < Q0; ++q) issue_one(q, jnn, buf);
        mfma_step(1, VA{});
    }
    dvq_dma_barrier();              // (the last iteration's look-ahead reads)
    // epilogue: the TM x 256 tile is staged as bf16 (512-byte rows, inside the two stages) and leaves in 16-byte stores
    const bool early_act = p.R == nullptr || p.res_mask;     // (residual / gate semantics of nt_epilogue_vec)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int jq = 0; jq < 4; ++jq) {
            const int lc = (wn * NT + nt) * 32 + 8 * jq + 4 * half;      // first of this lane's 4 columns
            float4 bq = {0.f, 0.f, 0.f, 0.f};
            if (p.bias_mode == 1 && n0 + lc < p.Ncols) bq = *reinterpret_cast<const float4*>(p.bias + n0 + lc);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int lr = (wm * MT + mt) * 32 + l31;
                const float brow = (p.bias_mode == 2 && m0 + lr < p.M) ? p.bias[m0 + lr] : 0.f;
                float v[4] = {acc[mt][nt][4 * jq] * p.alpha + bq.x + brow, acc[mt][nt][4 * jq + 1] * p.alpha + bq.y + brow,
                              acc[mt][nt][4 * jq + 2] * p.alpha + bq.z + brow, acc[mt][nt][4 * jq + 3] * p.alpha + bq.w + brow};
                if (early_act) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : v[k] * p.act_slope;
                }
                uint2 pk;
                pk.x = pack_bf16x2(v[0], v[1]);
                pk.y = pack_bf16x2(v[2], v[3]);
                const int chunk = ((wn * NT + nt) * 4 + jq) ^ (lr & 31);
                *reinterpret_cast<uint2*>(smem + lr * (WT * 2) + chunk * 16 + half * 8) = pk;
            }
        }
    }
    __syncthreads();
    T* __restrict__ Cg = reinterpret_cast<T*>(p.C) + bz * p.sC;
    const T* __restrict__ Rg = p.R ? reinterpret_cast<const T*>(p.R) + bz * p.sC : nullptr;
#pragma unroll 4
    for (int i = 0; i < (TM * WT / 8) / NTH; ++i) {
        const int q = tid + NTH * i;
        const int lr = q >> 5, ch = q & 31;
        const int row = m0 + lr, col = n0 + ch * 8;
        if (row >= p.M || col >= p.Ncols) continue;
        uint4 v = *reinterpret_cast<const uint4*>(smem + lr * (WT * 2) + ((ch ^ (lr & 31)) << 4));
        const int64_t o = (int64_t)row * p.ldc + col;
        if (Rg != nullptr) {
            const uint4 rv = *reinterpret_cast<const uint4*>(Rg + o);
            unsigned* pv = &v.x;
            const unsigned* pr = &rv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float lo = nt_res(p, __uint_as_float(pv[k] << 16), __uint_as_float(pr[k] << 16));
                const float hi = nt_res(p, __uint_as_float(pv[k] & 0xffff0000u), __uint_as_float(pr[k] & 0xffff0000u));
                pv[k] = pack_bf16x2(lo, hi);
            }
        }
        *reinterpret_cast<uint4*>(Cg + o) = v;
    }
#endif
}

// -------------------------------------------------------------------------------------------------
// 256 x 256 NT GEMM with an 8-phase main loop (the structure of cdna_hip_programming.md section 5's 256^2 template, written for the
// 32 x 32 x 16 MFMA): the DMA queue is NEVER drained inside the loop.  gemm_nt_wide_pipe_kernel above waits vmcnt(0) at every K slab
// (one slab in flight); here the operands move as HALF-TILES of 128 rows x 64 k (16 KiB = two 1-KiB pieces per wave), one per
// phase, seven of them ahead of the MFMAs, and the only wait is a counted vmcnt(6) once per K tile.
//   LDS     8 half-tile slots (128 KiB): K tile t lives in slots 4 (t & 1) + {0: B0, 1: A0, 2: B1, 3: A1} (A0 / A1 = rows 0..127 /
//           128..255 of the tile, B likewise for columns); rows are 128 B, 16-byte chunk c of row r at c ^ ((r >> 1) & 7) (the
//           permutation is applied to the DMA SOURCE address, the LDS image is lane-linear).
//   waves   8 = 2 (wr) x 4 (wc); a wave owns rows wr * 64 .. + 64 of BOTH A halves and columns wc * 32 .. + 32 of BOTH B halves, i.e.
//           four 64 x 32 quadrants (A half i, B half j), 2 MFMA tiles each.  A phase = one quadrant over the whole K tile (8 MFMAs):
//             phase 0 (A0, B0): reads 4 B0 + 8 A0 fragments      stages A1 of tile t + 1
//             phase 1 (A0, B1): reads 4 B1                        stages B0 of tile t + 2
//             phase 2 (A1, B1): reads 8 A1                        stages A0 of tile t + 2
//             phase 3 (A1, B0): reads nothing (B0 kept)           stages B1 of tile t + 2, then s_waitcnt vmcnt(6)
//           Every phase is [reads + 2 DMA pieces] s_barrier [8 MFMAs behind the compiler's counted lgkmcnt waits] s_barrier; the wr = 1 waves run ONE
//           barrier behind the wr = 0 waves, so on every SIMD one wave issues MFMAs while its partner issues reads and DMA.
//   RAW     a half-tile is read one phase (= at least two barriers, for both wave groups) after the vmcnt that retires it:
//           phase 3's vmcnt(6) leaves the three youngest half-tiles (B0, A0, B1 of t + 2) in flight -> tile t + 1 is complete.
//   WAR     a slot is re-staged two phases after its last read, except B0's (one phase): its four reads are issued first in phase 0
//           and retired by s_waitcnt lgkmcnt(8) BEFORE that phase's first barrier.
// K tiles past the end are re-fetches of the last tile into slots that are already dead; the queue is drained once, before the
// epilogue.  (Tried and removed, round 6: a PERSISTENT form whose half-tile stream runs on across tile boundaries and whose epilogue
// stores the accumulators straight from registers, 8 bytes per lane -- correct, but 16 % slower at 4096^3 and 8 - 18 % at K = 1024:
// 32 row-per-lane stores per wave are issue-bound, ~18 k cycles per tile, far more than the prologue + LDS-staged epilogue they replace.)  Epilogue: gemm_nt_wide_pipe_kernel's (packed bf16 tile through LDS, 16-byte stores).  Needs what that kernel needs.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void gemm_nt_8phase_kernel(NtParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using T = bf16_t;
    constexpr int HTB = 128 * GROW;                          // bytes of a half-tile slot
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int l31 = lane & 31, half = lane >> 5;
    const int wi = xcd_remap(blockIdx.x, p.gm * p.gn);
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * p.gn;
    const int grp = wi / per_group, rem = wi - grp * per_group;
    const int gsz = min(p.gm - grp * GROUP_M, GROUP_M);
    const int m0 = (grp * GROUP_M + rem % gsz) * WT, n0 = (rem / gsz) * WT;
    const int64_t bz = blockIdx.z;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(Ag), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(Bg), 0, 0x7fffffff, 0x00020000);
    // DMA: wave w sends pieces 2w, 2w + 1 (8 rows each) of every half-tile; lane -> row (lane >> 3), source chunk (lane & 7) ^ swizzle
    const int lrow = lane >> 3, cpos = lane & 7;
    int voA[2][2], voB[2][2];                               // [half][piece]: byte offset of this lane's 16 bytes in K tile 0
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int r = (2 * wave + e) * 8 + lrow;
            const int ch = (cpos ^ ((r >> 1) & 7)) * 8;
            voA[i][e] = (int)(((int64_t)min(m0 + i * 128 + r, p.M - 1) * p.lda + ch) * 2);
            voB[i][e] = (int)(((int64_t)min(n0 + i * 128 + r, p.Ncols - 1) * p.ldb + ch) * 2);
        }
    const int nk = p.Ktot / 64;
    // half-tile q of the stream order (0: B0, 1: A0, 2: B1, 3: A1) of K tile kt into slot `slot`
    auto stage = [&](auto qtag, int kt, int slot) {
        constexpr int q = decltype(qtag)::value;
        const int so = min(kt, nk - 1) * 128;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            auto dst = (__attribute__((address_space(3))) void*)(smem + slot * HTB + (2 * wave + e) * 1024);
            if constexpr ((q & 1) != 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, dst, 16, voA[q >> 1][e], so, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, voB[q >> 1][e], so, 0, 0);
        }
    };
    using Q0 = std::integral_constant<int, 0>;
    using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>;
    using Q3 = std::integral_constant<int, 3>;
    f32x16 acc[2][2][2];                                    // [A half][B half][row tile of the quadrant]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][f][r] = 0.f;
    // fragment addresses: byte offset of (row, 16-k step ks) inside a half-tile; `par` toggles between the two K-tile regions
    const int swz = ((l31 >> 1) & 7) ^ half;                 // chunk (2 ks + half) ^ ((row >> 1) & 7) = 2 ks ^ swz
    int ra[4], rb[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        ra[ks] = (wr * 64 + l31) * GROW + (((2 * ks) ^ swz) << 4);
        rb[ks] = (wc * 32 + l31) * GROW + (((2 * ks) ^ swz) << 4);
    }
    bf16x8 a[2][4], b0[4], b1[4];
    auto read_a = [&](int i) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int f = 0; f < 2; ++f) a[f][ks] = *reinterpret_cast<const bf16x8*>(smem + ra[ks] + (2 * i + 1) * HTB + f * 32 * GROW);
    };
    auto read_b = [&](int j, bf16x8 (&b)[4]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) b[ks] = *reinterpret_cast<const bf16x8*>(smem + rb[ks] + 2 * j * HTB);
    };
    // (measured at 8192^3, MI355X: the compiler's counted lgkmcnt waits between the MFMAs beat a blanket lgkmcnt(0) ahead of them, 1347
    // vs 1308 TFLOP/s, and s_setprio 1 around the MFMAs costs 1-2 % with 32 x 32 MFMAs -- 1375 without either)
    auto mfma8 = [&](int i, int j, bf16x8 (&b)[4]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int f = 0; f < 2; ++f)
                acc[i][j][f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[ks], a[f][ks], acc[i][j][f], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto bar = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    // prologue: K tile 0 and B0, A0, B1 of tile 1 (seven half-tiles); tile 0 has landed when at most three are outstanding
    stage(Q0{}, 0, 0);
    stage(Q1{}, 0, 1);
    stage(Q2{}, 0, 2);
    stage(Q3{}, 0, 3);
    stage(Q0{}, 1, 4);
    stage(Q1{}, 1, 5);
    stage(Q2{}, 1, 6);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    bar();
    if (wr == 1) bar();                                       // the second wave group runs one barrier behind
#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
        const int cur = (t & 1) * 4, nxt = cur ^ 4;
        // ---- phase 0: quadrant (A0, B0) ----
        read_b(0, b0);
        __builtin_amdgcn_sched_barrier(0);
        read_a(0);
        __builtin_amdgcn_sched_barrier(0);
        stage(Q3{}, t + 1, nxt + 3);
        asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");    // the four B0 reads have returned: slot B0 may be re-staged next phase
        bar();
        mfma8(0, 0, b0);
        bar();
        // ---- phase 1: quadrant (A0, B1) ----
        read_b(1, b1);
        __builtin_amdgcn_sched_barrier(0);
        stage(Q0{}, t + 2, cur + 0);
        bar();
        mfma8(0, 1, b1);
        bar();
        // ---- phase 2: quadrant (A1, B1) ----
        read_a(1);
        __builtin_amdgcn_sched_barrier(0);
        stage(Q1{}, t + 2, cur + 1);
        bar();
        mfma8(1, 1, b1);
        bar();
        // ---- phase 3: quadrant (A1, B0) ----
        stage(Q2{}, t + 2, cur + 2);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // all but the three youngest half-tiles: K tile t + 1 is complete
        bar();
        mfma8(1, 0, b0);
        bar();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {                      // the other K-tile region
            ra[ks] ^= 4 * HTB;
            rb[ks] ^= 4 * HTB;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (re-fetches past the end) nothing may land in the output staging
    if (wr == 0) bar();
    bar();
    // epilogue: the 256 x 256 tile is staged as bf16 (512-byte rows) and leaves in 16-byte stores
    const bool early_act = p.R == nullptr || p.res_mask;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int jq = 0; jq < 4; ++jq) {
            const int lc = j * 128 + wc * 32 + 8 * jq + 4 * half;        // first of this lane's 4 columns
            float4 bq = {0.f, 0.f, 0.f, 0.f};
            if (p.bias_mode == 1 && n0 + lc < p.Ncols) bq = *reinterpret_cast<const float4*>(p.bias + n0 + lc);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const int lr = i * 128 + wr * 64 + f * 32 + l31;
                    const float brow = (p.bias_mode == 2 && m0 + lr < p.M) ? p.bias[m0 + lr] : 0.f;
                    const f32x16& c = acc[i][j][f];
                    float v[4] = {c[4 * jq] * p.alpha + bq.x + brow, c[4 * jq + 1] * p.alpha + bq.y + brow,
                                  c[4 * jq + 2] * p.alpha + bq.z + brow, c[4 * jq + 3] * p.alpha + bq.w + brow};
                    if (early_act) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : v[k] * p.act_slope;
                    }
                    uint2 pk;
                    pk.x = pack_bf16x2(v[0], v[1]);
                    pk.y = pack_bf16x2(v[2], v[3]);
                    const int chunk = (j * 16 + wc * 4 + jq) ^ (lr & 31);
                    *reinterpret_cast<uint2*>(smem + lr * (WT * 2) + chunk * 16 + half * 8) = pk;
                }
        }
    }
    __syncthreads();
    T* __restrict__ Cg = reinterpret_cast<T*>(p.C) + bz * p.sC;
    const T* __restrict__ Rg = p.R ? reinterpret_cast<const T*>(p.R) + bz * p.sC : nullptr;
#pragma unroll 4
    for (int it = 0; it < (WT * WT / 8) / 512; ++it) {
        const int q = tid + 512 * it;
        const int lr = q >> 5, ch = q & 31;
        const int row = m0 + lr, col = n0 + ch * 8;
        if (row >= p.M || col >= p.Ncols) continue;
        uint4 v = *reinterpret_cast<const uint4*>(smem + lr * (WT * 2) + ((ch ^ (lr & 31)) << 4));
        const int64_t o = (int64_t)row * p.ldc + col;
        if (Rg != nullptr) {
            const uint4 rv = *reinterpret_cast<const uint4*>(Rg + o);
            unsigned* pv = &v.x;
            const unsigned* pr = &rv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float lo = nt_res(p, __uint_as_float(pv[k] << 16), __uint_as_float(pr[k] << 16));
                const float hi = nt_res(p, __uint_as_float(pv[k] & 0xffff0000u), __uint_as_float(pr[k] & 0xffff0000u));
                pv[k] = pack_bf16x2(lo, hi);
            }
        }
        *reinterpret_cast<uint4*>(Cg + o) = v;
    }
#endif
}

// -------------------------------------------------------------------------------------------------
// Pipelined implicit-GEMM convolution (bf16): the main loop of gemm_nt_wide_pipe_kernel with the A rows gathered through the
// convolution geometry -- strided, 4 x 4, 1 x 1 and small-map convolutions (forward: MODE_FWD) and their input gradients
// (MODE_TCONV; stride 2 by output parity class like igemm_nt_glds_kernel), i.e. everything the 3 x 3 halo kernel does not take.
// im2col never exists: a K slab is 64 channels of ONE tap, and for every row of the tile the source pixel of tap (u, v) is
// P(row) + sgn * (u * SW + v) -- a per-lane base offset fixed for the whole kernel plus a per-slab SCALAR offset, which is
// exactly what buffer_load ... lds takes (voffset / soffset).  Taps that fall outside the image (padding, tile tails) are a
// per-row bit mask computed once; a masked lane sends a voffset beyond the descriptor's range and the DMA writes zeros.
//   WMW x WNW waves of MT x NT 32 x 32 MFMA tiles: 4 x 2 x (2 x 4) = 256 rows x 256 columns (Cout >= 256),
//   4 x 2 x (2 x 2) = 256 x 128 (Cout = 128, or few row tiles), 8 x 1 x (2 x 2) = 512 x 64 (Cout <= 64),
//   2 x 2 x (2 x 2) = 128 x 128 with two workgroups per CU (short reductions: loads, MFMAs and stores of neighbours overlap).
// Needs Cs % 64 == 0, Ncols % 8 == 0, ldc % 8 == 0, operands below 2 GiB, at most 32 taps (per parity class).
// -------------------------------------------------------------------------------------------------
template <int WMW, int WNW, int MT, int NT, int MODE>
__global__ __launch_bounds__(64 * WMW * WNW, 2) void conv_nt_pipe_kernel(NtParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using T = bf16_t;
    constexpr int NWV = WMW * WNW, NTH = 64 * NWV;
    constexpr int TM = WMW * MT * 32, TN = WNW * NT * 32;   // tile rows (pixels) x columns (output channels)
    constexpr int NM = MT * NT, DS = MT + NT;                // MFMAs / fragment reads per 16-k step
    constexpr int NPA = TM / 8 / NWV, NPB = TN / 8 / NWV;    // DMA pieces (8 rows) per wave and K slab
    static_assert(NPA * 8 * NWV == TM && NPB * 8 * NWV == TN, "tile rows must split evenly over the waves' DMA pieces");
    constexpr int AOPB = TM * GROW, BOPB = TN * GROW, STG = AOPB + BOPB;
    constexpr int CPR = TN / 8;                              // 16-byte chunks per staged output row
    constexpr int VOFF_OOB = 0x7ffffff0;                     // beyond num_records: the DMA writes zeros
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WNW, wn = wave % WNW;
    const int l31 = lane & 31, half = lane >> 5;
    const int wi = xcd_remap(blockIdx.x, p.gm * p.gn);
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * p.gn;
    const int grp = wi / per_group, rem = wi - grp * per_group;
    const int gsz = min(p.gm - grp * GROUP_M, GROUP_M);
    int mtile = grp * GROUP_M + rem % gsz;
    const int n0 = (rem / gsz) * TN;
    const int Cs = (int)p.lda;
    const int KH = p.Ktot / Cs / p.KW;
    // class tap grid: all taps, or (stride-2 input gradient) the taps that reach output parity class pc
    const bool par = MODE == MODE_TCONV && p.par != 0;
    int pc = -1, Mrows = p.M, khc = 0, kwc = 0, nu = KH, nv = p.KW, qy = 0, qx = 0;
    if (par) {
        pc = mtile / p.par_tiles;
        mtile -= pc * p.par_tiles;
        Mrows = p.M >> 2;
        khc = ((pc >> 1) + p.pad_t) & 1;
        kwc = ((pc & 1) + p.pad_l) & 1;
        nu = (KH - khc + 1) >> 1;
        nv = (p.KW - kwc + 1) >> 1;
        qy = ((pc >> 1) + p.pad_t - khc) >> 1;
        qx = ((pc & 1) + p.pad_l - kwc) >> 1;
    }
    const int m0 = mtile * TM;
    constexpr int sgn = MODE == MODE_FWD ? 1 : -1;
    const int Dpix = MODE == MODE_FWD ? p.pad_t * p.SW + p.pad_l : 0;               // makes every lane's base pixel >= 0
    const int Dtap = MODE == MODE_FWD ? 0 : (nu - 1) * p.SW + nv - 1;                 // makes every tap's shift >= 0
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) - (int64_t)(Dpix + Dtap) * Cs;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B);
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(Ag), 0, 0x7fffffe0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(Bg), 0, 0x7fffffff, 0x00020000);
    const int lrow = lane >> 3, cpos = lane & 7;
    int aoff[NPA], boff[NPB];
    unsigned amask[NPA];
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        const int trow = (wave * NPA + i) * 8 + lrow;
        const int m = m0 + trow;
        const bool rok = m < Mrows;
        const int mm = rok ? m : 0;
        const int dw_ = par ? p.DW >> 1 : p.DW, dh_ = par ? p.DH >> 1 : p.DH;
        const int hw = dh_ * dw_;
        const int n = mm / hw, r2 = mm - n * hw;
        const int y = r2 / dw_, x = r2 - y * dw_;
        int Py, Px;
        if constexpr (MODE == MODE_FWD) {
            Py = y * p.stride - p.pad_t;
            Px = x * p.stride - p.pad_l;
        } else {
            Py = par ? y + qy : y + p.pad_t;
            Px = par ? x + qx : x + p.pad_l;
        }
        const int pix = (n * p.SH + Py) * p.SW + Px + Dpix;
        aoff[i] = (pix * Cs + (cpos ^ ((trow >> 1) & 7)) * 8) * 2;
        unsigned xm = 0, msk = 0;
        for (int v = 0; v < nv; ++v) xm |= ((unsigned)(Px + sgn * v) < (unsigned)p.LW ? 1u : 0u) << v;
        for (int u = 0; u < nu; ++u)
            if ((unsigned)(Py + sgn * u) < (unsigned)p.LH) msk |= xm << (u * nv);
        amask[i] = rok ? msk : 0u;
    }
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
        const int trow = (wave * NPB + i) * 8 + lrow;
        boff[i] = (int)(((int64_t)min(n0 + trow, p.Ncols - 1) * p.ldb + (cpos ^ ((trow >> 1) & 7)) * 8) * 2);
    }
    // K slab -> (tap t = u * nv + v, 64-channel chunk c): scalar state advanced slab by slab (no divisions in the loop)
    const int spt = Cs >> 6;
    const int nk = nu * nv * spt;
    struct Slab {
        int t, c, u, v;
    };
    auto advance = [&](Slab s) {
        if (++s.c == spt) {
            s.c = 0;
            ++s.t;
            if (++s.v == nv) {
                s.v = 0;
                ++s.u;
            }
        }
        return s;
    };
    auto so_a = [&](const Slab& s) { return ((sgn * (s.u * p.SW + s.v) + Dtap) * Cs + s.c * 64) * 2; };
    auto so_b = [&](const Slab& s) { return (((khc + (par ? 2 : 1) * s.u) * p.KW + kwc + (par ? 2 : 1) * s.v) * Cs + s.c * 64) * 2; };
    constexpr int ND = NPA + NPB;
    auto issue_one = [&](int q, const Slab& s, int buf) {    // DMA instruction q of a K slab: A piece q, or B piece q - NPA
        if (q < NPA) {
            const int vo = ((amask[q] >> s.t) & 1u) ? aoff[q] : VOFF_OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsA, (__attribute__((address_space(3))) void*)(smem + buf * STG + (wave * NPA + q) * 8 * GROW), 16, vo, so_a(s), 0, 0);
        } else {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsB, (__attribute__((address_space(3))) void*)(smem + buf * STG + AOPB + (wave * NPB + q - NPA) * 8 * GROW), 16,
                boff[q - NPA], so_b(s), 0, 0);
        }
    };
    f32x16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int swz = (l31 >> 1) & 7;
    const char* pa;
    const char* pb;
    auto set_stage = [&](int buf) {
        pa = smem + buf * STG + (wm * (MT * 32) + l31) * GROW;
        pb = smem + buf * STG + AOPB + (wn * (NT * 32) + l31) * GROW;
    };
    bf16x8 a[2][MT], b[2][NT];
    auto load_frags = [&](int ks, int slot) {                 // in the order the MFMAs consume them
        const int off = ((ks * 2 + half) ^ swz) << 4;
        a[slot][0] = *reinterpret_cast<const bf16x8*>(pa + off);
#pragma unroll
        for (int t = 0; t < NT; ++t) b[slot][t] = *reinterpret_cast<const bf16x8*>(pb + t * 32 * GROW + off);
#pragma unroll
        for (int t = 1; t < MT; ++t) a[slot][t] = *reinterpret_cast<const bf16x8*>(pa + t * 32 * GROW + off);
    };
    auto mfma_step = [&](int slot, auto vm_tag) {
        constexpr int VM = decltype(vm_tag)::value;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[slot][nt], a[slot][mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (2 * i < DS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            else if (i - DS / 2 < VM) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    constexpr int Q0 = (ND + 2) / 3, Q1 = Q0 + (ND - Q0 + 1) / 2;     // DMA of a slab over three steps: [0, Q0) | [Q0, Q1) | [Q1, ND)
    using V0 = std::integral_constant<int, 0>;
    using VA = std::integral_constant<int, Q0>;
    using VB = std::integral_constant<int, Q1 - Q0>;
    using VC = std::integral_constant<int, ND - Q1>;
    Slab s1{0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < ND; ++q) issue_one(q, s1, 0);
    if (nk > 1) s1 = advance(s1);                             // slab j + 1
    Slab s2 = nk > 2 ? advance(s1) : s1;                      // slab j + 2
    dvq_dma_barrier();
    set_stage(0);
    load_frags(0, 0);
#pragma unroll
    for (int q = 0; q < Q0; ++q) issue_one(q, s1, 1);
#pragma unroll 1
    for (int j = 0; j < nk; ++j) {
        const int buf = j & 1;
        __builtin_amdgcn_sched_barrier(0);
        load_frags(1, 1);
#pragma unroll
        for (int q = Q0; q < Q1; ++q) issue_one(q, s1, buf ^ 1);
        mfma_step(0, VB{});
        load_frags(2, 0);
#pragma unroll
        for (int q = Q1; q < ND; ++q) issue_one(q, s1, buf ^ 1);
        mfma_step(1, VC{});
        load_frags(3, 1);
        mfma_step(0, V0{});
        dvq_dma_barrier();          // every wave has its reads of this slab behind it and its pieces of the next one landed
        set_stage(buf ^ 1);
        load_frags(0, 0);
#pragma unroll
        for (int q = 0; q < Q0; ++q) issue_one(q, s2, buf);   // (past the end: harmless re-fetches into dead stages)
        mfma_step(1, VA{});
        s1 = s2;
        if (j + 3 < nk) s2 = advance(s2);
    }
    dvq_dma_barrier();              // (the last iteration's look-ahead reads and DMA)
    // epilogue: the TM x TN tile is staged as bf16 (rows of TN * 2 bytes, inside the two stages) and leaves in 16-byte stores
    const bool early_act = p.R == nullptr || p.res_mask;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int jq = 0; jq < 4; ++jq) {
            const int lc = (wn * NT + nt) * 32 + 8 * jq + 4 * half;      // first of this lane's 4 columns
            float4 bq = {0.f, 0.f, 0.f, 0.f};
            if (p.bias_mode == 1 && n0 + lc < p.Ncols) bq = *reinterpret_cast<const float4*>(p.bias + n0 + lc);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int lr = (wm * MT + mt) * 32 + l31;
                float v[4] = {acc[mt][nt][4 * jq] + bq.x, acc[mt][nt][4 * jq + 1] + bq.y, acc[mt][nt][4 * jq + 2] + bq.z,
                              acc[mt][nt][4 * jq + 3] + bq.w};
                if (early_act) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : v[k] * p.act_slope;
                }
                uint2 pk;
                pk.x = pack_bf16x2(v[0], v[1]);
                pk.y = pack_bf16x2(v[2], v[3]);
                const int chunk = ((wn * NT + nt) * 4 + jq) ^ (lr & (CPR - 1));
                *reinterpret_cast<uint2*>(smem + lr * (TN * 2) + chunk * 16 + half * 8) = pk;
            }
        }
    }
    __syncthreads();
    T* __restrict__ Cg = reinterpret_cast<T*>(p.C);
    const T* __restrict__ Rg = reinterpret_cast<const T*>(p.R);
#pragma unroll 4
    for (int i = 0; i < (TM * CPR) / NTH; ++i) {
        const int q = tid + NTH * i;
        const int lr = q / CPR, ch = q % CPR;
        const int row = m0 + lr, col = n0 + ch * 8;
        if (row >= Mrows || col >= p.Ncols) continue;
        uint4 v = *reinterpret_cast<const uint4*>(smem + lr * (TN * 2) + ((ch ^ (lr & (CPR - 1))) << 4));
        const int64_t o = (par ? par_out_row(p, pc, row) : (int64_t)row) * p.ldc + col;
        if (Rg != nullptr) {
            const uint4 rv = *reinterpret_cast<const uint4*>(Rg + o);
            unsigned* pv = &v.x;
            const unsigned* pr = &rv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float lo = nt_res(p, __uint_as_float(pv[k] << 16), __uint_as_float(pr[k] << 16));
                const float hi = nt_res(p, __uint_as_float(pv[k] & 0xffff0000u), __uint_as_float(pr[k] & 0xffff0000u));
                pv[k] = pack_bf16x2(lo, hi);
            }
        }
        *reinterpret_cast<uint4*>(Cg + o) = v;
    }
#endif
}

// -------------------------------------------------------------------------------------------------
// Skinny NT GEMM (bf16, M <= 32 rows): the single-token Linear layers of K/V-cached sampling.  The product is bound by
// streaming the weight matrix B [N][K] once, so the tiling is by WEIGHT ROWS: a workgroup owns 32 rows of B, its waves split K,
// and each wave feeds 32x32x16 MFMAs straight from global memory -- MFMA A operand = 32 weight rows x 16 k (one 16-byte load
// per lane), B operand = the (zero-padded) 32 activation rows x 16 k (L1/L2 resident) -- no LDS staging, no tile of 128 rows
// that is 75 - 97% padding.  The waves' partial accumulators are added in LDS.  (The 128 x 128 kernel put these products on
// 8 - 32 workgroups for 20 - 85 us each; 24 layers x 6 products made the sampler GPU-bound at 8 ms per token.)
// -------------------------------------------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(64 * NW) void gemm_nt_skinny_kernel(NtParams p) {
    using T = bf16_t;
    __shared__ float red[NW][32][33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int n0 = blockIdx.x * 32;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A);
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B);
    const int ksteps = (p.Ktot + 15) / 16;
    const int per = (ksteps + NW - 1) / NW;
    const int ks0 = wave * per, ks1 = min(ksteps, ks0 + per);
    const bool wok = n0 + l31 < p.Ncols, xok = l31 < p.M;
    const T* wrow = Bg + (int64_t)(wok ? n0 + l31 : 0) * p.ldb + 8 * half;
    const T* xrow = Ag + (int64_t)(xok ? l31 : 0) * p.lda + 8 * half;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const uint4 z = make_uint4(0, 0, 0, 0);
    // 16 k-steps of loads in flight per wave (16 KiB of weights): with 4 the kernel spent one HBM round trip per 4 KiB and wave --
    // 7.9 us for a 1024 x 1024 layer, 21 us for 4096-long reductions (rocprofv3 of the sampler; round 3)
    for (int kc = ks0; kc < ks1; kc += 16) {
        uint4 wv[16], xv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int ks = kc + u;
            const bool kok = ks < ks1 && ks * 16 + 8 * half < p.Ktot;   // K % 8 == 0: a lane's 8 elements are all in or out
            wv[u] = (wok && kok) ? *reinterpret_cast<const uint4*>(wrow + ks * 16) : z;
            xv[u] = (xok && kok) ? *reinterpret_cast<const uint4*>(xrow + ks * 16) : z;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wv[u]), __builtin_bit_cast(bf16x8, xv[u]), acc, 0, 0, 0);
    }
    // acc[r]: weight row (r & 3) + 8 (r >> 2) + 4 half, activation row l31
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][(r & 3) + 8 * (r >> 2) + 4 * half][l31] = acc[r];
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += 64 * NW) {
        const int m = e >> 5, nn = e & 31;                              // consecutive threads -> consecutive output columns
        if (m >= p.M || n0 + nn >= p.Ncols) continue;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += red[w][nn][m];
        v *= p.alpha;
        if (p.bias_mode == 1) v += p.bias[n0 + nn];
        reinterpret_cast<T*>(p.C)[(int64_t)m * p.ldc + n0 + nn] = f32_to_bf16(v);
    }
}

// -------------------------------------------------------------------------------------------------
// naive kernels (any shape; used for validation, tiny shapes and as the loud fallback of DVQ_IMPL_NAIVE)
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ void naive_nt_kernel(NtParams p) {
    const int64_t total = (int64_t)p.M * p.Ncols;
    const int64_t bz = blockIdx.z;
    const T* Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    T* Cg = reinterpret_cast<T*>(p.C) + bz * p.sC;
    const T* Rg = p.R ? reinterpret_cast<const T*>(p.R) + bz * p.sC : nullptr;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(e / p.Ncols), col = (int)(e % p.Ncols);
        float acc = 0.f;
        if (p.mode == MODE_GEMM) {
            for (int k = 0; k < p.Ktot; ++k)
                acc = fmaf(ElemIO<T>::load(Ag + (int64_t)m * p.lda + k), ElemIO<T>::load(Bg + (int64_t)col * p.ldb + k), acc);
        } else {
            const int Cs = (int)p.lda;
            const int taps = p.Ktot / Cs;
            const int hw = p.DH * p.DW;
            const int n = m / hw, rem = m % hw, y = rem / p.DW, x = rem % p.DW;
            for (int tap = 0; tap < taps; ++tap) {
                const int kh = tap / p.KW, kw = tap % p.KW;
                int64_t off;
                if (p.mode == MODE_FWD) {
                    const int ih = y * p.stride - p.pad_t + kh, iw = x * p.stride - p.pad_l + kw;
                    if ((unsigned)ih >= (unsigned)p.LH || (unsigned)iw >= (unsigned)p.LW) continue;
                    off = (((int64_t)n * p.SH + (ih >> p.up)) * p.SW + (iw >> p.up)) * Cs;
                } else {
                    const int t = y + p.pad_t - kh, v = x + p.pad_l - kw;
                    if (t < 0 || v < 0 || t % p.stride || v % p.stride) continue;
                    const int oh = t / p.stride, ow = v / p.stride;
                    if (oh >= p.LH || ow >= p.LW) continue;
                    off = (((int64_t)n * p.SH + oh) * p.SW + ow) * Cs;
                }
                const T* a = Ag + off;
                const T* b = Bg + (int64_t)col * p.ldb + (int64_t)tap * Cs;
                for (int c = 0; c < Cs; ++c) acc = fmaf(ElemIO<T>::load(a + c), ElemIO<T>::load(b + c), acc);
            }
        }
        float v = acc * p.alpha;
        if (p.bias_mode == 1) v += p.bias[col];
        if (p.bias_mode == 2) v += p.bias[m];
        const int64_t o = (int64_t)m * p.ldc + col;
        if (Rg) {
            const float rr = ElemIO<T>::load(Rg + o);
            if (p.res_mask) v *= rr > 0.f ? 1.f : p.mask_slope;
            else v += rr;
        }
        v = v > 0.f ? v : v * p.act_slope;
        ElemIO<T>::store(Cg + o, v);
    }
}

// -------------------------------------------------------------------------------------------------
// launch helpers: per kernel an eligibility predicate and a launcher; launch_nt / launch_tn try the kernels in priority order
// -------------------------------------------------------------------------------------------------
// every MFMA kernel: whole vectors along K on both operands
template <typename T>
bool nt_mfma_ok(const NtParams& p) {
    constexpr int VN = Vec<T>::N;
    bool mfma_ok = p.Ktot % VN == 0 && p.ldb % VN == 0 && p.lda % VN == 0 && (p.stride == 1 || p.stride == 2);
    if (p.mode == MODE_GEMM) mfma_ok = mfma_ok && (p.sA % VN == 0) && (p.sB % VN == 0);
    return mfma_ok;
}

// The four 256-wide kernels (bf16, nt_mfma_ok shapes): plain GEMMs under every code that reaches them; convolutions only under the
// automatic choice; a residual only under the automatic choice, DVQ_IMPL_WIDE_PIPE and DVQ_IMPL_8PHASE.
// 256 x 256 macro tiles pay off on long reductions that fill the chip for several rounds (8192^3: 1036 vs 812 TFLOP/s);
// on the StackGPT shapes (K = 1024 .. 4096, 324 .. 1296 tiles) the 128 x 128 kernel is faster (tools/gemm_probe.py),
// so the automatic choice is conservative.
bool nt_wide_ok(const NtParams& p, int impl) {
    // a 1 x 1 / stride 1 / unpadded convolution (forward, or input gradient through the transposed pack) IS a plain GEMM
    const bool conv1x1 = p.mode != MODE_GEMM && p.Ktot == (int)p.lda && p.KW == 1 && p.stride == 1 && p.pad_t == 0 && p.pad_l == 0 &&
                         p.up == 0 && p.LH == p.DH && p.LW == p.DW && p.par == 0;
    return (p.mode == MODE_GEMM || (conv1x1 && impl == DVQ_IMPL_AUTO)) &&
           (p.R == nullptr || impl == DVQ_IMPL_AUTO || impl == DVQ_IMPL_WIDE_PIPE || impl == DVQ_IMPL_8PHASE) &&
           p.ldc % Vec<bf16_t>::N == 0 && p.M >= 256 && p.Ncols >= 256;
}

// the pipelined main loops among them (wide_pipe, 8-phase): faster than both the 128 x 128 kernel and the plain wide one on every
// tools/gemm_probe.py shape (679 / 775 / 865 / 870 / 1141 against 575 / 640 / 594 / 779 / 840 and 535 / 593 / 636 / 695 / 1050 TFLOP/s)
bool nt_wide_pipe_ok(const NtParams& p) {
    return p.Ncols % 8 == 0 && p.Ktot % 64 == 0 && (int64_t)p.M * p.lda < (1ll << 30) && (int64_t)p.Ncols * p.ldb < (1ll << 30);
}

// the 8-phase main loop (counted vmcnt, seven half-tiles ahead): long reductions over several rounds of tiles -- 8192^3 runs at
// 1375 TFLOP/s against 1129 for the kernel below and 1332 for hipBLASLt's best solution on the same box (tools/gemm8p_probe.py);
// its prologue (112 KiB before the first MFMA) and lock-step rounds lose at K <= 4096 / a single round (4096^3: 1181 vs 1280)
int launch_nt_8phase(NtParams p, int64_t batch, hipStream_t s) {
    const int64_t wgm = cdiv64(p.M, WT), wgn = cdiv64(p.Ncols, WT);
    p.gm = (int)wgm;
    p.gn = (int)wgn;
    dvq_note_kernel("gemm_nt_8phase_kernel");
    dvq_ensure_dynamic_lds((const void*)gemm_nt_8phase_kernel, 8 * 128 * GROW);
    gemm_nt_8phase_kernel<<<dim3((unsigned)(wgm * wgn), 1, (unsigned)batch), dim3(512), 8 * 128 * GROW, s>>>(p);
    DVQ_CHECK_LAUNCH("gemm_nt_8phase");
    return DVQ_OK;
}

// experiment: 4 waves x (4 x 4 tiles), one wave per SIMD
int launch_nt_wide_pipe4(NtParams p, int64_t batch, hipStream_t s) {
    const int64_t wgm = cdiv64(p.M, WT), wgn = cdiv64(p.Ncols, WT);
    p.gm = (int)wgm;
    p.gn = (int)wgn;
    dvq_note_kernel("gemm_nt_wide_pipe_kernel");
    dvq_ensure_dynamic_lds((const void*)gemm_nt_wide_pipe_kernel<2, 2, 4>, 2 * WSTAGEB);
    gemm_nt_wide_pipe_kernel<2, 2, 4><<<dim3((unsigned)(wgm * wgn), 1, (unsigned)batch), dim3(256), 2 * WSTAGEB, s>>>(p);
    DVQ_CHECK_LAUNCH("gemm_nt_wide_pipe4");
    return DVQ_OK;
}

// rows: 256 or 192 as the impl code asks, 0 = whichever needs less tile-row-time over the 256 CUs (rounds x rows)
int launch_nt_wide_pipe(NtParams p, int64_t batch, int rows, hipStream_t s) {
    const int64_t wgm = cdiv64(p.M, WT), wgn = cdiv64(p.Ncols, WT);
    dvq_note_kernel("gemm_nt_wide_pipe_kernel");
    const int64_t wgm192 = cdiv64(p.M, 192);
    const int64_t cost256 = cdiv64(wgm * wgn * batch, 256) * 256, cost192 = cdiv64(wgm192 * wgn * batch, 256) * 192;
    p.gn = (int)wgn;
    if (rows == 192 || (rows == 0 && cost192 * 10 < cost256 * 8)) {
        p.gm = (int)wgm192;
        dvq_ensure_dynamic_lds((const void*)gemm_nt_wide_pipe_kernel<2, 2, 3>, 2 * (192 + 256) * GROW);
        gemm_nt_wide_pipe_kernel<2, 2, 3><<<dim3((unsigned)(wgm192 * wgn), 1, (unsigned)batch), dim3(256), 2 * (192 + 256) * GROW, s>>>(p);
    } else {
        p.gm = (int)wgm;
        dvq_ensure_dynamic_lds((const void*)gemm_nt_wide_pipe_kernel<4, 2, 2>, 2 * WSTAGEB);
        gemm_nt_wide_pipe_kernel<4, 2, 2><<<dim3((unsigned)(wgm * wgn), 1, (unsigned)batch), dim3(512), 2 * WSTAGEB, s>>>(p);
    }
    DVQ_CHECK_LAUNCH("gemm_nt_wide_pipe");
    return DVQ_OK;
}

int launch_nt_wide(NtParams p, int64_t batch, hipStream_t s) {
    const int64_t wgm = cdiv64(p.M, WT), wgn = cdiv64(p.Ncols, WT);
    p.gm = (int)wgm;
    p.gn = (int)wgn;
    dvq_note_kernel("gemm_nt_wide_kernel");
    dvq_ensure_dynamic_lds((const void*)gemm_nt_wide_kernel, 2 * WSTAGEB);
    gemm_nt_wide_kernel<<<dim3((unsigned)(wgm * wgn), 1, (unsigned)batch), dim3(512), 2 * WSTAGEB, s>>>(p);
    DVQ_CHECK_LAUNCH("gemm_nt_wide");
    return DVQ_OK;
}

// pipelined implicit-GEMM convolution (conv_nt_pipe_kernel, bf16): everything with 64-channel K slabs
bool nt_conv_pipe_ok(const NtParams& p) {
    const int khn = p.mode != MODE_GEMM && p.lda > 0 && p.KW > 0 ? (int)(p.Ktot / p.lda / p.KW) : 0;
    const bool s2par = p.mode == MODE_TCONV && p.stride == 2;
    bool pipe_ok = p.mode != MODE_GEMM && p.up == 0 && p.lda % 64 == 0 && p.ldb == p.Ktot &&
                   p.Ncols % 8 == 0 && p.ldc % 8 == 0 && (p.stride == 1 || p.stride == 2) && khn >= 1 && khn * p.KW <= 16 &&
                   (int64_t)khn * p.KW * p.lda == p.Ktot && p.bias_mode != 2 && p.alpha == 1.f &&
                   ((int64_t)p.SH * p.SW * (p.M / ((int64_t)p.DH * p.DW)) + 2 * (4 * (int64_t)p.SW + 4)) * p.lda * 2 < 0x7fe00000ll &&
                   (int64_t)p.Ncols * p.ldb * 2 < 0x7fe00000ll && p.M % ((int64_t)p.DH * p.DW) == 0;
    if (s2par) pipe_ok = pipe_ok && p.DH % 2 == 0 && p.DW % 2 == 0 && p.M % 4 == 0;
    return pipe_ok;
}

int launch_nt_conv_pipe(NtParams p, hipStream_t s) {
    // tile choice (tools/conv_bench.py sweeps): 256 x 256 when that fills >= 3/4 of a round of 256 CUs,
    // else 128 x 128 at two workgroups per CU; thin outputs 512 x 64
    const int cfg = p.Ncols <= 16 ? 4 : p.Ncols <= 64 ? 3 : p.Ncols <= 128 ? 4 : (cdiv64(p.M, 256) * cdiv64(p.Ncols, 256) < 192 ? 4 : 1);
    const int tm = cfg == 3 ? 512 : cfg == 4 ? 128 : 256, tn = cfg == 1 ? 256 : cfg == 3 ? 64 : 128;
    if (p.mode == MODE_TCONV && p.stride == 2) {
        p.par = 1;
        p.par_tiles = (int)cdiv64(p.M / 4, tm);
        p.gm = 4 * p.par_tiles;
    } else {
        p.par = 0;
        p.gm = (int)cdiv64(p.M, tm);
    }
    p.gn = (int)cdiv64(p.Ncols, tn);
    const int lds = 2 * (tm + tn) * GROW;
    const dim3 grid((unsigned)((int64_t)p.gm * p.gn));
    auto go = [&](auto kern) {
        dvq_ensure_dynamic_lds((const void*)kern, lds);
        kern<<<grid, dim3(cfg == 4 ? 256 : 512), lds, s>>>(p);
    };
    dvq_note_kernel("conv_nt_pipe_kernel");
    const bool fwd = p.mode == MODE_FWD;
    if (cfg == 4) fwd ? go(conv_nt_pipe_kernel<2, 2, 2, 2, MODE_FWD>) : go(conv_nt_pipe_kernel<2, 2, 2, 2, MODE_TCONV>);
    else if (cfg == 1) fwd ? go(conv_nt_pipe_kernel<4, 2, 2, 4, MODE_FWD>) : go(conv_nt_pipe_kernel<4, 2, 2, 4, MODE_TCONV>);
    else fwd ? go(conv_nt_pipe_kernel<8, 1, 2, 2, MODE_FWD>) : go(conv_nt_pipe_kernel<8, 1, 2, 2, MODE_TCONV>);
    DVQ_CHECK_LAUNCH("conv_nt_pipe");
    return DVQ_OK;
}

// 128 x 128 LDS-DMA kernel: every nt_mfma_ok shape
template <typename T>
int launch_nt_glds(NtParams p, int64_t batch, hipStream_t s) {
    constexpr int VN = Vec<T>::N;
    const bool tapu = p.mode != MODE_GEMM && ((p.lda / VN) % 8) == 0;
    if (p.mode == MODE_TCONV && p.stride == 2 && p.up == 0 && tapu && p.DH % 2 == 0 && p.DW % 2 == 0 && p.ldc % VN == 0) {
        // stride-2 input gradient: rows grouped by output parity class, each class contracts over its own taps only
        p.par = 1;
        p.par_tiles = (int)cdiv64(p.M / 4, TILE);
        p.gm = 4 * p.par_tiles;
    }
    dim3 grid((unsigned)(p.gm * p.gn), 1, (unsigned)batch);
    dvq_note_kernel("igemm_nt_glds_kernel");
    auto go = [&](auto kern) {
        dvq_ensure_dynamic_lds((const void*)kern, 2 * GSTAGEB);
        kern<<<grid, dim3(256), 2 * GSTAGEB, s>>>(p);
    };
    constexpr bool F32 = sizeof(T) == 4;
    if (F32 && p.split3) {              // fp32x3: the split-bf16 instantiations (separate kernels: the exact-fp32 code is untouched)
        if (p.mode == MODE_GEMM) go(igemm_nt_glds_kernel<T, MODE_GEMM, false, F32>);
        else if (p.mode == MODE_FWD && tapu) go(igemm_nt_glds_kernel<T, MODE_FWD, true, F32>);
        else if (p.mode == MODE_FWD) go(igemm_nt_glds_kernel<T, MODE_FWD, false, F32>);
        else if (tapu) go(igemm_nt_glds_kernel<T, MODE_TCONV, true, F32>);
        else go(igemm_nt_glds_kernel<T, MODE_TCONV, false, F32>);
    } else if (p.mode == MODE_GEMM) go(igemm_nt_glds_kernel<T, MODE_GEMM, false>);
    else if (p.mode == MODE_FWD && tapu) go(igemm_nt_glds_kernel<T, MODE_FWD, true>);
    else if (p.mode == MODE_FWD) go(igemm_nt_glds_kernel<T, MODE_FWD, false>);
    else if (tapu) go(igemm_nt_glds_kernel<T, MODE_TCONV, true>);
    else go(igemm_nt_glds_kernel<T, MODE_TCONV, false>);
    DVQ_CHECK_LAUNCH("igemm_nt_glds");
    return DVQ_OK;
}

// register-staged 128 x 128 kernel
template <typename T>
int launch_nt_regstage(NtParams p, int64_t batch, hipStream_t s) {
    dim3 grid((unsigned)(p.gm * p.gn), 1, (unsigned)batch);
    dvq_note_kernel("igemm_nt_kernel");
    dvq_ensure_dynamic_lds((const void*)igemm_nt_kernel<T>, 2 * STAGEB);
    igemm_nt_kernel<T><<<grid, dim3(256), 2 * STAGEB, s>>>(p);
    DVQ_CHECK_LAUNCH("igemm_nt");
    return DVQ_OK;
}

template <typename T>
int launch_nt_naive(NtParams p, int64_t batch, hipStream_t s) {
    int64_t total = (int64_t)p.M * p.Ncols;
    unsigned blocks = (unsigned)(cdiv64(total, 256) < 16384 ? cdiv64(total, 256) : 16384);
    dvq_note_kernel("naive_nt_kernel");
    naive_nt_kernel<T><<<dim3(blocks, 1, (unsigned)batch), dim3(256), 0, s>>>(p);
    DVQ_CHECK_LAUNCH("naive_nt");
    return DVQ_OK;
}

}  // namespace

// Priority order: 8-phase, 4-wave pipe, wide pipe, plain wide, pipelined convolution, 128 x 128 LDS-DMA, register-staged, naive.
// A preferred code stands in for the automatic heuristic of its kernel only; a required code returns DVQ_ESHAPE on a shape its kernel
// does not run.
template <typename T>
int launch_nt(NtParams p, int64_t batch, int impl, hipStream_t s) {
    p.split3 = sizeof(T) == 4 && dvq_fp32_split() != 0;
    p.gm = (int)cdiv64(p.M, TILE);
    p.gn = (int)cdiv64(p.Ncols, TILE);
    const bool mfma_ok = nt_mfma_ok<T>(p);
    const bool auto_or_preferred = impl == DVQ_IMPL_AUTO || impl_preferred(impl);
    DVQ_REQUIRE(mfma_ok || impl < DVQ_IMPL_MFMA || auto_or_preferred || impl == DVQ_IMPL_CONV_PIPE, DVQ_ESHAPE,
                "igemm_nt: MFMA path needs K, lda, ldb multiples of %d (K=%d lda=%lld ldb=%lld) and stride 1/2", Vec<T>::N,
                p.Ktot, (long long)p.lda, (long long)p.ldb);
    const bool use_mfma = impl == DVQ_IMPL_MFMA || impl == DVQ_IMPL_REGSTAGE ||
                          ((auto_or_preferred || impl == DVQ_IMPL_CONV_PIPE) && mfma_ok && (int64_t)p.M * p.Ncols >= 1024);
    if constexpr (sizeof(T) == 2) {
        const int64_t wtiles = cdiv64(p.M, WT) * cdiv64(p.Ncols, WT) * batch;
        const bool wide_ok = auto_or_preferred && mfma_ok && nt_wide_ok(p, impl);
        const bool wide_pipe_ok = wide_ok && nt_wide_pipe_ok(p);
        if (wide_pipe_ok && (impl == DVQ_IMPL_8PHASE || (impl == DVQ_IMPL_AUTO && p.Ktot >= 4096 && wtiles >= 512)))
            return launch_nt_8phase(p, batch, s);
        if (wide_pipe_ok && impl == DVQ_IMPL_WIDE_PIPE_4WAVE) return launch_nt_wide_pipe4(p, batch, s);
        if (wide_pipe_ok && (impl == DVQ_IMPL_WIDE_PIPE || impl == DVQ_IMPL_WIDE_PIPE_192 || (impl == DVQ_IMPL_AUTO && wtiles >= 128)))
            return launch_nt_wide_pipe(p, batch, impl == DVQ_IMPL_WIDE_PIPE_192 ? 192 : impl == DVQ_IMPL_WIDE_PIPE ? 256 : 0, s);
        if (wide_ok && p.mode == MODE_GEMM && p.R == nullptr && (impl == DVQ_IMPL_WIDE || (p.Ktot >= 8192 && wtiles >= 768)))
            return launch_nt_wide(p, batch, s);
        const bool conv_pipe_ok = (impl == DVQ_IMPL_AUTO || impl == DVQ_IMPL_CONV_PIPE) && nt_conv_pipe_ok(p);
        DVQ_REQUIRE(!(impl == DVQ_IMPL_CONV_PIPE && !conv_pipe_ok), DVQ_ESHAPE, "igemm_nt: shape not eligible for the pipelined convolution kernel");
        if (conv_pipe_ok) return launch_nt_conv_pipe(p, s);
    }
    if (use_mfma && impl != DVQ_IMPL_REGSTAGE) return launch_nt_glds<T>(p, batch, s);
    if (use_mfma) return launch_nt_regstage<T>(p, batch, s);
    return launch_nt_naive<T>(p, batch, s);
}

template int launch_nt<float>(NtParams, int64_t, int, hipStream_t);
template int launch_nt<bf16_t>(NtParams, int64_t, int, hipStream_t);

// single-token Linear layers of the sampler: weight-streaming kernel (notes no family)
int launch_nt_skinny(const NtParams& p, hipStream_t s) {
    const unsigned blocks = (unsigned)cdiv64(p.Ncols, 32);
    // waves split K so that each has at most ~16 k-steps = one batch of loads
    if (p.Ktot > 2048) gemm_nt_skinny_kernel<16><<<dim3(blocks), dim3(1024), 0, s>>>(p);
    else if (p.Ktot > 1024) gemm_nt_skinny_kernel<8><<<dim3(blocks), dim3(512), 0, s>>>(p);
    else gemm_nt_skinny_kernel<4><<<dim3(blocks), dim3(256), 0, s>>>(p);
    DVQ_CHECK_LAUNCH("gemm_nt_skinny");
    return DVQ_OK;
}

}  // namespace igemm
