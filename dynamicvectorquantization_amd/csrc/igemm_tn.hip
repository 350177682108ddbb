// TN side of the implicit-GEMM convolution / batched GEMM (map of the files: igemm.hip):
//   C[i][j] += sum_m A[m][i] * B[m][j]     weight gradients and generic TN products, fp32 output
// Kernels (register-staged, transpose-read, patch, wide-pipe, 8-phase, reduce, naive, deterministic fold), predicates, launchers and launch_tn.
#include <type_traits>

#include "igemm.h"
#include "igemm_dev.h"

namespace igemm {
namespace {

// -------------------------------------------------------------------------------------------------
// TN kernel (wgrad / generic).  C fp32, accumulated with atomics; grid.y splits the reduction.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t tn_c_offset(const TnParams& p, int row, int tap, int col) {
    return p.c_oihw ? ((int64_t)row * p.Jc + col) * p.taps + tap : (int64_t)row * p.ldc + (int64_t)tap * p.Jc + col;
}

template <typename T, bool CONV, bool S3 = false>
__global__ __launch_bounds__(256, 2) void igemm_tn_kernel(TnParams p) {
    constexpr int VN = Vec<T>::N;      // 8 (bf16) / 4 (fp32): block edge of the register transpose
    constexpr int BK = Vec<T>::BK;     // 64 / 32 reduction rows per stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int per_split = p.itiles * p.jtiles * p.taps;
    int bx = xcd_remap(blockIdx.x, per_split * p.nsplit);
    const int split = bx / per_split;       // all tiles/taps of one split are consecutive -> same XCD, same time
    bx -= split * per_split;
    const int it = bx % p.itiles;
    bx /= p.itiles;
    const int jt = bx % p.jtiles;
    const int tap = bx / p.jtiles;
    const int i0 = it * TILE, j0 = jt * TILE;
    const int64_t bz = blockIdx.z;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const int mbeg = split * p.m_per_split;
    const int mend = min(p.Mred, mbeg + p.m_per_split);
    const int kh = tap / p.KW, kw = tap - kh * p.KW;

    // thread -> (operand, VN x VN block).  bf16: 128 blocks per operand -> half the threads each;
    // fp32: 256 blocks per operand -> every thread does both.
    constexpr int NBLK_COL = TILE / VN;          // 16 / 32 blocks across the i (or j) dimension
    constexpr bool SPLIT_OPS = sizeof(T) == 2;
    const int u = SPLIT_OPS ? (tid & 127) : tid;
    const int mb = u / NBLK_COL, cb = u % NBLK_COL;   // m block (rows mb*VN..), column block
    const bool doA = !SPLIT_OPS || tid < 128;
    const bool doB = !SPLIT_OPS || tid >= 128;
    const bool do_bias = p.colsumA != nullptr && tap == 0 && jt == 0 && doA;

    uint4 ra[VN], rb[VN];
    float bsum[VN];
#pragma unroll
    for (int c = 0; c < VN; ++c) bsum[c] = 0.f;

    // conv gather: pixel coordinates of this thread's first row, advanced by BK rows per stage (no divisions
    // in the loop); pixel offsets stay 32-bit, one 64-bit multiply-add per row forms the element offset
    int gn = 0, gy = 0, gx = 0;
    if constexpr (CONV) {
        const int hw = p.DH * p.DW;
        const int mm0 = min(mbeg + mb * VN, p.Mred - 1);
        gn = mm0 / hw;
        const int rem = mm0 - gn * hw;
        gy = rem / p.DW;
        gx = rem - gy * p.DW;
    }
    const int colA = i0 + cb * VN, colB = j0 + cb * VN;
    auto g_load = [&](int ms) {   // ms: first reduction row of the stage
        const int mrow = ms + mb * VN;
        if (doA) {
            const T* src = Ag + (int64_t)mrow * p.lda + colA;
#pragma unroll
            for (int r = 0; r < VN; ++r) {
                const bool ok = mrow + r < mend && colA < p.I;
                ra[r] = ok ? *reinterpret_cast<const uint4*>(src + (int64_t)r * p.lda) : make_uint4(0, 0, 0, 0);
            }
        }
        if (doB) {
            if constexpr (!CONV) {
                const T* src = Bg + (int64_t)mrow * p.ldb + colB;
#pragma unroll
                for (int r = 0; r < VN; ++r) {
                    const bool ok = mrow + r < mend && colB < p.J;
                    rb[r] = ok ? *reinterpret_cast<const uint4*>(src + (int64_t)r * p.ldb) : make_uint4(0, 0, 0, 0);
                }
            } else {
                int n = gn, y = gy, x = gx;
#pragma unroll
                for (int r = 0; r < VN; ++r) {
                    bool ok = mrow + r < mend && colB < p.J;
                    const int ih = y * p.stride - p.pad_t + kh, iw = x * p.stride - p.pad_l + kw;
                    ok = ok && (unsigned)ih < (unsigned)p.LH && (unsigned)iw < (unsigned)p.LW;
                    const int pix = (n * p.SH + (ih >> p.up)) * p.SW + (iw >> p.up);
                    rb[r] = ok ? *reinterpret_cast<const uint4*>(Bg + (int64_t)pix * p.ldb + colB) : make_uint4(0, 0, 0, 0);
                    if (++x == p.DW) {
                        x = 0;
                        if (++y == p.DH) {
                            y = 0;
                            ++n;
                        }
                    }
                }
                // advance the walk by one stage (BK rows)
                gx += BK;
                while (gx >= p.DW) {
                    gx -= p.DW;
                    if (++gy == p.DH) {
                        gy = 0;
                        ++gn;
                    }
                }
            }
        }
    };
    // register transpose + LDS store: column c of the block becomes LDS row (cb*VN + c), 16-B chunk mb,
    // stored at chunk position mb ^ swz_tn(row) of an unpadded 128-B row (conflict-free, see SWZ_TN)
    auto store_op = [&](const uint4 (&rg)[VN], char* sbase) {
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                unsigned w[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const unsigned x0 = (&rg[2 * v].x)[c >> 1], x1 = (&rg[2 * v + 1].x)[c >> 1];
                    w[v] = (c & 1) ? ((x0 >> 16) | (x1 & 0xffff0000u)) : ((x0 & 0xffffu) | (x1 << 16));
                }
                const int row = cb * VN + c;
                *reinterpret_cast<uint4*>(sbase + row * GROW + ((mb ^ swz_tn(row)) << 4)) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int row = cb * VN + c;
                *reinterpret_cast<uint4*>(sbase + row * GROW + ((mb ^ swz_tn(row)) << 4)) =
                    make_uint4((&rg[0].x)[c], (&rg[1].x)[c], (&rg[2].x)[c], (&rg[3].x)[c]);
            }
        }
    };
    auto s_store = [&](int buf) {
        if (doA) {
            if (do_bias) {
#pragma unroll
                for (int r = 0; r < VN; ++r) {
                    if constexpr (sizeof(T) == 2) {
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            const unsigned wv = (&ra[r].x)[c >> 1];
                            bsum[c] += __uint_as_float((c & 1) ? (wv & 0xffff0000u) : (wv << 16));
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c) bsum[c] += __uint_as_float((&ra[r].x)[c]);
                    }
                }
            }
            store_op(ra, smem + buf * GSTAGEB);
        }
        if (doB) store_op(rb, smem + buf * GSTAGEB + GOPB);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = (mend - mbeg + BK - 1) / BK;
    if (nk > 0) {
        g_load(mbeg);
        s_store(0);
        __syncthreads();
        for (int j = 0; j < nk; ++j) {
            const int buf = j & 1;
            if (j + 1 < nk) g_load(mbeg + (j + 1) * BK);
            mma_stage_swz<T, SWZ_TN, S3>(smem + buf * GSTAGEB, smem + buf * GSTAGEB + GOPB, acc, wm, wn, lane);
            if (j + 1 < nk) s_store(buf ^ 1);
            __syncthreads();
        }
    }

    float* __restrict__ Cg = p.C + bz * p.sC;
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int col = j0 + wn * 64 + nt * 32 + l31;
        if (col >= p.Jc) continue;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < p.I) {
                    if (p.dws != nullptr) p.dws[(int64_t)split * p.dws_stride + tn_c_offset(p, row, tap, col)] = acc[mt][nt][r];
                    else atomicAdd(Cg + tn_c_offset(p, row, tap, col), acc[mt][nt][r]);
                }
            }
    }
    if (p.det) {
        // deterministic mode: the BK / VN row blocks of the workgroup park their column sums in LDS (the stages have been consumed:
        // the main loop ends on a barrier), thread `col` adds them in block order and is the column's only writer of this split
        if (p.colsumA == nullptr || tap != 0 || jt != 0) return;
        constexpr int NMB = (SPLIT_OPS ? 128 : 256) / NBLK_COL;
        float* sb = reinterpret_cast<float*>(smem);              // [NMB][TILE]
        if (doA) {
#pragma unroll
            for (int c = 0; c < VN; ++c) sb[mb * TILE + cb * VN + c] = bsum[c];
        }
        __syncthreads();
        if (tid < TILE && i0 + tid < p.I) {
            float t = 0.f;
#pragma unroll
            for (int m = 0; m < NMB; ++m) t += sb[m * TILE + tid];
            if (p.dws_bias != nullptr) p.dws_bias[(int64_t)split * p.I + i0 + tid] = t;
            else p.colsumA[i0 + tid] += t;                       // (unsplit launch)
        }
        return;
    }
    if (do_bias) {
#pragma unroll
        for (int c = 0; c < VN; ++c) {
            const int col = i0 + cb * VN + c;
            if (col < p.I) atomicAdd(p.colsumA + col, bsum[c]);
        }
    }
}

// -------------------------------------------------------------------------------------------------
// TN kernel, bf16, LDS-DMA staging + hardware transpose reads (ds_read_b64_tr_b16).
// Both operand tiles stay in their natural [reduction row m][channel] layout (256-B rows filled by
// global_load_lds), and the MFMA fragments -- which need 8 consecutive m for one channel per lane -- are
// formed by two transpose reads each: within a 16-lane group, lanes 4r..4r+3 address row r (8 B each) of a
// 4-row x 16-channel block and lane i receives column i (probed on hardware, tools/probes/tr_probe.hip).
// Swizzle: 16-B chunk c of row r lives at chunk position c ^ ((r & 3) << 2), so the 4 rows x 64 B that one
// 32-lane half reads cover all 64 banks exactly once.
// -------------------------------------------------------------------------------------------------
constexpr int TROW = 256;              // LDS row bytes: 128 bf16 channels
constexpr int TOPB = 64 * TROW;        // 64 reduction rows per stage and operand
constexpr int TSTAGEB = 2 * TOPB;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

template <bool CONV>
__global__ __launch_bounds__(256, 2) void igemm_tn_tr_kernel(TnParams p) {
    using T = bf16_t;
    constexpr int BK = 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const bool thin = CONV && p.thin != 0;
    const int per_split = p.itiles * p.jtiles * (thin ? 1 : p.taps);
    int bx = xcd_remap(blockIdx.x, per_split * p.nsplit);
    const int split = bx / per_split;
    bx -= split * per_split;
    const int it = bx % p.itiles;
    bx /= p.itiles;
    const int jt = bx % p.jtiles;
    const int tap = bx / p.jtiles;
    const int i0 = it * TILE, j0 = jt * TILE;
    const int64_t bz = blockIdx.z;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* __restrict__ Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const T* zero = reinterpret_cast<const T*>(g_zero_page);
    const int mbeg = split * p.m_per_split;
    const int mend = min(p.Mred, mbeg + p.m_per_split);
    int kh = tap / p.KW, kw = tap - kh * p.KW;

    // ---- loader: DMA piece i of this wave = stage rows (wave*4 + i)*4 .. +3, lane -> (row lr, chunk position) ----
    const int lr = lane >> 4, cpos = lane & 15;
    const int cg = cpos ^ (lr << 2);               // source chunk of this lane (stage rows of a piece are 4-aligned)
    const int colA = i0 + cg * 8;
    int colB = j0 + cg * 8;
    const bool cokA = colA < p.I;
    bool cokB = colB < p.J;
    if (thin) {                                    // this lane's chunk is tap `cg`: all 8 (padded) input channels of one tap
        kh = cg / p.KW;
        kw = cg - kh * p.KW;
        colB = 0;
        cokB = cg < p.taps;
    }
    int gn[4], gy[4], gx[4];
    if constexpr (CONV) {
        const int hw = p.DH * p.DW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = min(mbeg + (wave * 4 + i) * 4 + lr, p.Mred - 1);
            gn[i] = m / hw;
            const int rem = m - gn[i] * hw;
            gy[i] = rem / p.DW;
            gx[i] = rem - gy[i] * p.DW;
        }
    }
    auto issue = [&](int ms, int buf) {            // ms: first reduction row of the stage
        char* sa = smem + buf * TSTAGEB + wave * 16 * TROW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = ms + (wave * 4 + i) * 4 + lr;
            const bool okm = m < mend;
            const T* srcA = (okm && cokA) ? Ag + (int64_t)m * p.lda + colA : zero;
            const T* srcB;
            if constexpr (!CONV) {
                srcB = (okm && cokB) ? Bg + (int64_t)m * p.ldb + colB : zero;
            } else {
                const int ih = gy[i] * p.stride - p.pad_t + kh, iw = gx[i] * p.stride - p.pad_l + kw;
                const bool ok = okm && cokB && (unsigned)ih < (unsigned)p.LH && (unsigned)iw < (unsigned)p.LW;
                const int pix = (gn[i] * p.SH + (ih >> p.up)) * p.SW + (iw >> p.up);
                srcB = ok ? Bg + (int64_t)pix * p.ldb + colB : zero;
                gx[i] += BK;                       // walk to the next stage (BK rows further), no divisions
                while (gx[i] >= p.DW) {
                    gx[i] -= p.DW;
                    if (++gy[i] == p.DH) {
                        gy[i] = 0;
                        ++gn[i];
                    }
                }
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcA,
                                             (__attribute__((address_space(3))) void*)(sa + i * 4 * TROW), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcB,
                                             (__attribute__((address_space(3))) void*)(sa + TOPB + i * 4 * TROW), 16, 0, 0);
        }
    };

    // ---- fragment addressing (per lane constants) ----
    const int g = lane >> 4, li = lane & 15;
    const int frow = 8 * (g >> 1) + (li >> 2);                 // + ks*16 + 4*t (multiples of 4: swizzle term unchanged)
    const int fz = ((li >> 2) & 3) << 2;
    int offA[2], offB[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int chA = wm * 8 + t * 4 + 2 * (g & 1) + ((li & 3) >> 1);
        const int chB = wn * 8 + t * 4 + 2 * (g & 1) + ((li & 3) >> 1);
        offA[t] = frow * TROW + ((chA ^ fz) << 4) + (li & 1) * 8;
        offB[t] = frow * TROW + ((chB ^ fz) << 4) + (li & 1) * 8;
    }
    const bool do_bias = p.colsumA != nullptr && tap == 0 && jt == 0 && wn == 0;
    float bsum[2] = {0.f, 0.f};

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    auto frag = [&](const char* base, int off, int ks) -> bf16x8 {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + off + (ks * 16) * TROW));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + off + (ks * 16 + 4) * TROW));
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = lo[j];
            v[4 + j] = hi[j];
        }
        return v;
    };

    const int nk = (mend - mbeg + BK - 1) / BK;
    if (nk > 0) {
        issue(mbeg, 0);
        dvq_dma_barrier();
        for (int j = 0; j < nk; ++j) {
            const int buf = j & 1;
            if (j + 1 < nk) issue(mbeg + (j + 1) * BK, buf ^ 1);
            const char* sA = smem + buf * TSTAGEB;
            const char* sB = sA + TOPB;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                bf16x8 a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = frag(sA, offA[t], ks);
                    b[t] = frag(sB, offB[t], ks);
                }
                if (do_bias) {
                    // (element-wise extraction from a __bf16 vector mis-compiles to element 0 here: go through uint4)
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const uint4 u = __builtin_bit_cast(uint4, a[t]);
                        bsum[t] += (__uint_as_float(u.x << 16) + __uint_as_float(u.x & 0xffff0000u)) +
                                   (__uint_as_float(u.y << 16) + __uint_as_float(u.y & 0xffff0000u)) +
                                   (__uint_as_float(u.z << 16) + __uint_as_float(u.z & 0xffff0000u)) +
                                   (__uint_as_float(u.w << 16) + __uint_as_float(u.w & 0xffff0000u));
                    }
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
            }
            dvq_dma_barrier();
        }
    }

    float* __restrict__ Cg = p.C + bz * p.sC;
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        int col = j0 + wn * 64 + nt * 32 + l31, ctap = tap;
        if (thin) {
            ctap = col >> 3;
            col &= 7;
            if (ctap >= p.taps) continue;
        }
        if (col >= p.Jc) continue;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < p.I) {
                    if (p.dws != nullptr) p.dws[(int64_t)split * p.dws_stride + tn_c_offset(p, row, ctap, col)] = acc[mt][nt][r];
                    else atomicAdd(Cg + tn_c_offset(p, row, ctap, col), acc[mt][nt][r]);
                }
            }
    }
    if (do_bias) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float v = bsum[t] + __shfl_xor(bsum[t], 32, 64);    // the two lane halves hold different m
            const int col = i0 + wm * 64 + t * 32 + l31;
            if (half == 0 && col < p.I) {
                if (p.dws_bias != nullptr) p.dws_bias[(int64_t)split * p.I + col] = v;
                else atomicAdd(p.colsumA + col, v);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Convolution weight gradient on PATCHES (bf16): dW[co][tap][ci] += sum_px dy[px][co] x[gather(px, tap)][ci], 128 x 128 tile per
// (tap, co tile, ci tile) like igemm_tn_tr_kernel, but a 64-row stage is an 8 x 8 PATCH of output pixels instead of 64 consecutive
// pixels (the sum over pixels has no order).  Inside a patch the source address of a lane's 16 bytes is
//     [patch origin: scalar, rebuilt per stage on the scalar unit]  +  [pixel of the lane inside the patch: one 32-bit constant],
// for dy and for the gathered x rows alike (stride, padding, tap offset and the folded nearest x2 upsampling are part of the
// constant), so a stage's DMA costs 3 vector instructions per x piece (the padding mask: per-lane edge flags & the patch's edge code)
// and none per dy piece.  igemm_tn_tr_kernel decodes every row's pixel and builds two 64-bit addresses per piece and stage, ~40
// vector instructions x 8 pieces per 16 MFMAs: it is bound by that arithmetic (0.12 of the MFMA peak on the step's shapes).
// Fragment reads run one 16-row step ahead of their MFMAs.  Output rows / columns past DH / DW (31 x 31 PatchGAN maps) are
// masked like padding.  Split over patch ranges, fp32 atomics.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void conv_tn_patch_kernel(TnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using T = bf16_t;
    constexpr int OOB = 0x7ffffff0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int per_split = p.itiles * p.jtiles * p.taps;
    int bx = xcd_remap(blockIdx.x, per_split * p.nsplit);
    const int split = bx / per_split;
    bx -= split * per_split;
    const int it = bx % p.itiles;
    bx /= p.itiles;
    const int jt = bx % p.jtiles;
    const int tap = bx / p.jtiles;
    const int i0 = it * TILE, j0 = jt * TILE;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const T* Ag = reinterpret_cast<const T*>(p.A);
    const T* Bg = reinterpret_cast<const T*>(p.B);
    const int PH = (p.DH + 7) >> 3, PW = (p.DW + 7) >> 3;            // patches per image column / row
    const int npatch = (p.Mred / (p.DH * p.DW)) * PH * PW;
    const int pbeg = split * p.m_per_split, pend = min(npatch, pbeg + p.m_per_split);      // (m_per_split counts patches here)

    // ---- per-lane constants of this wave's 4 + 4 DMA pieces (stage rows (wave * 4 + i) * 4 + lr = patch pixel (r >> 3, r & 7)) ----
    const int lr = lane >> 4, cpos = lane & 15;
    const int cg = cpos ^ (lr << 2);
    const int colA = i0 + cg * 8, colB = j0 + cg * 8;
    // even bias of the lane-relative input coordinates (keeps them non-negative; even so that the >> up of the sum splits)
    const int by = (p.pad_t + 1) & ~1, bxp = (p.pad_l + 1) & ~1;
    int voA[4], voB[4], flA[4], flB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 4 + lr, ly = r >> 3, lx = r & 7;
        voA[i] = colA < p.I ? (int)(((int64_t)(ly * p.DW + lx) * p.lda + colA) * 2) : OOB;
        flA[i] = (ly >= p.DH - 8 * (PH - 1) ? 2 : 0) | (lx >= p.DW - 8 * (PW - 1) ? 8 : 0);
        const int ry = ly * p.stride - p.pad_t + kh, rx = lx * p.stride - p.pad_l + kw;      // relative to the patch origin * stride
        voB[i] = colB < p.J ? (int)(((int64_t)(((ry + by) >> p.up) * p.SW + ((rx + bxp) >> p.up)) * p.ldb + colB) * 2) : OOB;
        flB[i] = (ry < 0 ? 1 : 0) | (8 * (PH - 1) * p.stride + ry >= p.LH ? 2 : 0) | (rx < 0 ? 4 : 0) | (8 * (PW - 1) * p.stride + rx >= p.LW ? 8 : 0);
    }
    int sn, spy, spx;                               // the next patch to be issued
    {
        const int ppi = PH * PW;
        sn = pbeg / ppi;
        const int rem = pbeg - sn * ppi;
        spy = rem / PW;
        spx = rem - spy * PW;
    }
    auto make_rsrc = [&](const T* base) {
        const unsigned long long a = (unsigned long long)base;
        int32x4 r;
        r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
        r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
        r.z = 0x7fff0000;
        r.w = 0x00020000;
        return r;
    };
    auto issue = [&](int buf) {
        const int oy0 = spy * 8, ox0 = spx * 8;
        const int32x4 rsA = make_rsrc(Ag + (((int64_t)sn * p.DH + oy0) * p.DW + ox0) * p.lda);
        // (for patches at the top / left edge this base lies before the image: only masked lanes would go there)
        const int32x4 rsB = make_rsrc(Bg + (((int64_t)sn * p.SH + ((oy0 * p.stride - by) >> p.up)) * p.SW + ((ox0 * p.stride - bxp) >> p.up)) * p.ldb);
        const int edge = (spy == 0 ? 1 : 0) | (spy == PH - 1 ? 2 : 0) | (spx == 0 ? 4 : 0) | (spx == PW - 1 ? 8 : 0);
        char* sa = smem + buf * TSTAGEB + wave * 16 * TROW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int va = (flA[i] & edge) ? OOB : voA[i];
            const int vb = ((flB[i] | flA[i]) & edge) ? OOB : voB[i];
            const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)(sa + i * 4 * TROW));
            // (inline assembly: see gemm_tn_wide_pipe_kernel -- the compiler would drain every LDS-DMA before the first transpose read)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(la), "v"(va), "s"(rsA));
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(la + (unsigned)TOPB), "v"(vb), "s"(rsB));
        }
        if (++spx == PW) {
            spx = 0;
            if (++spy == PH) {
                spy = 0;
                ++sn;
            }
        }
    };

    // ---- fragment addressing (per lane constants, as igemm_tn_tr_kernel) ----
    const int g = lane >> 4, li = lane & 15;
    const int frow = 8 * (g >> 1) + (li >> 2);
    const int fz = ((li >> 2) & 3) << 2;
    int offA[2], offB[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int chA = wm * 8 + t * 4 + 2 * (g & 1) + ((li & 3) >> 1);
        const int chB = wn * 8 + t * 4 + 2 * (g & 1) + ((li & 3) >> 1);
        offA[t] = frow * TROW + ((chA ^ fz) << 4) + (li & 1) * 8;
        offB[t] = frow * TROW + ((chB ^ fz) << 4) + (li & 1) * 8;
    }
    const bool do_bias = p.colsumA != nullptr && tap == 0 && jt == 0 && wn == 0;
    float bsum[2] = {0.f, 0.f};
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    auto frag = [&](const char* base, int off, int ks) -> bf16x8 {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + off + (ks * 16) * TROW));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + off + (ks * 16 + 4) * TROW));
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = lo[j];
            v[4 + j] = hi[j];
        }
        return v;
    };

    if (pbeg < pend) {
        issue(0);
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        __syncthreads();
        for (int j = pbeg; j < pend; ++j) {
            const int buf = (j - pbeg) & 1;
            if (j + 1 < pend) issue(buf ^ 1);
            const char* sA = smem + buf * TSTAGEB;
            const char* sB = sA + TOPB;
            bf16x8 a[2][2], b[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[0][t] = frag(sA, offA[t], 0);
                b[0][t] = frag(sB, offB[t], 0);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks + 1 < 4) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        a[(ks + 1) & 1][t] = frag(sA, offA[t], ks + 1);
                        b[(ks + 1) & 1][t] = frag(sB, offB[t], ks + 1);
                    }
                }
                if (do_bias) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const uint4 u = __builtin_bit_cast(uint4, a[ks & 1][t]);
                        bsum[t] += (__uint_as_float(u.x << 16) + __uint_as_float(u.x & 0xffff0000u)) +
                                   (__uint_as_float(u.y << 16) + __uint_as_float(u.y & 0xffff0000u)) +
                                   (__uint_as_float(u.z << 16) + __uint_as_float(u.z & 0xffff0000u)) +
                                   (__uint_as_float(u.w << 16) + __uint_as_float(u.w & 0xffff0000u));
                    }
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks & 1][mt], b[ks & 1][nt], acc[mt][nt], 0, 0, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
            __syncthreads();
        }
    }

    float* __restrict__ Cg = p.C;
    const int l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int col = j0 + wn * 64 + nt * 32 + l31;
        if (col >= p.Jc) continue;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < p.I) {
                    if (p.dws != nullptr) p.dws[(int64_t)split * p.dws_stride + tn_c_offset(p, row, tap, col)] = acc[mt][nt][r];
                    else atomicAdd(Cg + tn_c_offset(p, row, tap, col), acc[mt][nt][r]);
                }
            }
    }
    if (do_bias) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float v = bsum[t] + __shfl_xor(bsum[t], 32, 64);
            const int col = i0 + wm * 64 + t * 32 + l31;
            if (half == 0 && col < p.I) {
                if (p.dws_bias != nullptr) p.dws_bias[(int64_t)split * p.I + col] = v;
                else atomicAdd(p.colsumA + col, v);
            }
        }
    }
#endif
}

// -------------------------------------------------------------------------------------------------
// Wide TN GEMM (bf16 weight gradients of the Linear layers: C[i][j] += sum_m A[m][i] B[m][j]): 256 x 256 tile, 8 waves x (2 x 4)
// MFMA tiles, 64 reduction rows per stage (2 x 32 KiB, rows of 512 B), operands in their natural [m][column] layout with the
// K-contiguous fragments formed by ds_read_b64_tr_b16 (as igemm_tn_tr_kernel), split over m with fp32 atomics.  Main loop pipelined
// like gemm_nt_wide_pipe_kernel; the DMA is issued from INLINE ASSEMBLY (buffer_load_dwordx4 ... lds through an SGPR descriptor,
// one fixed 32-bit lane offset per piece, the stage as scalar offset): the compiler orders every ds_read_b64_tr behind all LDS-DMA
// it knows to be pending (s_waitcnt vmcnt(0) before the first transpose read), which would serialise the prefetch of the next
// stage with the reads of this one; pieces it does not know of are drained by hand before the barrier that publishes them.
// Rows past the end of a split read as zero through the descriptor's bound; columns past I / J load neighbouring data that ends
// up in accumulator columns nobody stores.
// -------------------------------------------------------------------------------------------------
constexpr int WTROW = 512;                     // LDS row bytes: 256 bf16 columns
constexpr int WTOPB = 64 * WTROW;              // 64 reduction rows per stage and operand
constexpr int WTSTG = 2 * WTOPB;

__global__ __launch_bounds__(512, 2) void gemm_tn_wide_pipe_kernel(TnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using T = bf16_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                 // 4 x 2 waves: 64 rows (i) x 128 columns (j) each
    const int per_split = p.itiles * p.jtiles;
    int bx = xcd_remap(blockIdx.x, per_split * p.nsplit);
    const int split = bx / per_split;
    bx -= split * per_split;
    const int it = bx % p.itiles, jt = bx / p.itiles;
    const int i0 = it * 256, j0 = jt * 256;
    const int64_t bz = blockIdx.z;
    const T* Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const int mbeg = split * p.m_per_split;
    const int mend = min(p.Mred, mbeg + p.m_per_split);
    const int nk = (mend - mbeg + 63) / 64;

    auto make_rsrc = [&](const T* base, int64_t bytes) {
        const unsigned long long a = (unsigned long long)base;
        int32x4 r;
        r.x = (int)(unsigned)a;
        r.y = (int)(unsigned)(a >> 32);
        r.z = (int)bytes;                                    // reads at or past this byte offset return zero
        r.w = 0x00020000;
        r.x = __builtin_amdgcn_readfirstlane(r.x);
        r.y = __builtin_amdgcn_readfirstlane(r.y);
        r.z = __builtin_amdgcn_readfirstlane(r.z);
        return r;
    };
    const int32x4 rsA = make_rsrc(Ag, (int64_t)mend * p.lda * 2), rsB = make_rsrc(Bg, (int64_t)mend * p.ldb * 2);
    // DMA instruction q of this wave: q < 4 -> A, else B; stage rows (wave * 4 + (q & 3)) * 2 + (lane >> 5); a lane at chunk position
    // pos of its row fetches source chunk pos ^ ((row & 3) << 2) (the swizzle the transpose reads undo)
    int voff[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int row = (wave * 4 + (q & 3)) * 2 + (lane >> 5);
        const int cg = (lane & 31) ^ ((row & 3) << 2);
        voff[q] = q < 4 ? (int)(((int64_t)(mbeg + row) * p.lda + i0 + cg * 8) * 2) : (int)(((int64_t)(mbeg + row) * p.ldb + j0 + cg * 8) * 2);
    }
    const int sstepA = (int)(64 * p.lda * 2), sstepB = (int)(64 * p.ldb * 2);      // bytes per stage
    auto dma = [&](int q, int j, int buf) {
        char* dst = smem + buf * WTSTG + (q < 4 ? 0 : WTOPB) + (wave * 4 + (q & 3)) * 2 * WTROW;
        const unsigned l = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)dst);
        const int so = __builtin_amdgcn_readfirstlane(j * (q < 4 ? sstepA : sstepB));
        if (q < 4)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" : : "s"(l), "v"(voff[q]), "s"(rsA), "s"(so));
        else
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" : : "s"(l), "v"(voff[q]), "s"(rsB), "s"(so));
    };

    // fragment addressing (per lane constants, as igemm_tn_tr_kernel): a 16-lane group reads 4 rows x 16 columns per ds_read_b64_tr
    const int g = lane >> 4, li = lane & 15;
    const int frow = 8 * (g >> 1) + (li >> 2);                 // + ks*16 (+4 for the second read)
    const int fz = ((li >> 2) & 3) << 2;
    int offA[2], offB[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) offA[t] = frow * WTROW + (((wm * 8 + t * 4 + 2 * (g & 1) + ((li & 3) >> 1)) ^ fz) << 4) + (li & 1) * 8;
#pragma unroll
    for (int t = 0; t < 4; ++t) offB[t] = frow * WTROW + (((wn * 16 + t * 4 + 2 * (g & 1) + ((li & 3) >> 1)) ^ fz) << 4) + (li & 1) * 8;
    const bool do_bias = p.colsumA != nullptr && jt == 0 && wn == 0;
    float bsum[2] = {0.f, 0.f};

    f32x16 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    auto frag = [&](const char* base, int off, int ks) -> bf16x8 {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + off + (ks * 16) * WTROW));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + off + (ks * 16 + 4) * WTROW));
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    bf16x8 a[2][2], b[2][4];
    // fragments of step ks of stage `buf` into `slot`, in the order the MFMAs consume them, with up to NDMA DMA instructions
    // (q0, q0 + 1, ...) of K stage jd placed between them (inline assembly keeps its place among the LDS reads)
    auto load_frags = [&](int buf, int ks, int slot, int q0, int ndma, int jd, int bufd) {
        const char* sA = smem + buf * WTSTG;
        const char* sB = sA + WTOPB;
        a[slot][0] = frag(sA, offA[0], ks);
        if (ndma > 0) dma(q0, jd, bufd);
        b[slot][0] = frag(sB, offB[0], ks);
        if (ndma > 1) dma(q0 + 1, jd, bufd);
        b[slot][1] = frag(sB, offB[1], ks);
        if (ndma > 2) dma(q0 + 2, jd, bufd);
        b[slot][2] = frag(sB, offB[2], ks);
        b[slot][3] = frag(sB, offB[3], ks);
        a[slot][1] = frag(sA, offA[1], ks);
    };
    auto mfma_step = [&](int slot) {
        if (do_bias) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const uint4 u = __builtin_bit_cast(uint4, a[slot][t]);
                bsum[t] += (__uint_as_float(u.x << 16) + __uint_as_float(u.x & 0xffff0000u)) +
                           (__uint_as_float(u.y << 16) + __uint_as_float(u.y & 0xffff0000u)) +
                           (__uint_as_float(u.z << 16) + __uint_as_float(u.z & 0xffff0000u)) +
                           (__uint_as_float(u.w << 16) + __uint_as_float(u.w & 0xffff0000u));
            }
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[slot][mt], b[slot][nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {                          // 12 transpose reads: two behind each of the first six MFMAs
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (i < 6) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    if (nk > 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) dma(q, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        __syncthreads();
        load_frags(0, 0, 0, 0, 3, nk > 1 ? 1 : 0, 1);          // + DMA 0..2 of stage 1
#pragma unroll 1
        for (int j = 0; j < nk; ++j) {
            const int buf = j & 1;
            const int jn = j + 1 < nk ? j + 1 : nk - 1;        // (past the end: harmless re-fetches into dead stages)
            const int jnn = j + 2 < nk ? j + 2 : nk - 1;
            __builtin_amdgcn_sched_barrier(0);
            load_frags(buf, 1, 1, 3, 3, jn, buf ^ 1);          // DMA 3..5 of the next stage
            mfma_step(0);
            load_frags(buf, 2, 0, 6, 2, jn, buf ^ 1);          // DMA 6, 7
            mfma_step(1);
            load_frags(buf, 3, 1, 0, 0, 0, 0);
            mfma_step(0);
            asm volatile("s_waitcnt vmcnt(0)" : : : "memory");  // the hand-issued pieces of the next stage
            __syncthreads();
            load_frags(buf ^ 1, 0, 0, 0, 3, jnn, buf);         // first reads of the next stage; DMA 0..2 of the one after it
            mfma_step(1);
        }
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    }

    const int l31 = lane & 31, half = lane >> 5;
    if (p.ws != nullptr) {
        // Cross-XCD fp32 atomics resolve at the memory side and cost far more than plain stores: with a workspace every workgroup
        // stores its 256 x 256 partial tile with ordinary coalesced writes and gemm_tn_wide_reduce_kernel folds the splits into C
        float* tile = p.ws + ((int64_t)split * per_split + it + (int64_t)jt * p.itiles) * 65536;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    tile[(wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 256 + wn * 128 + nt * 32 + l31] = acc[mt][nt][r];
        if (do_bias) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float v = bsum[t] + __shfl_xor(bsum[t], 32, 64);
                if (half == 0) p.ws_bias[((int64_t)split * p.itiles + it) * 256 + wm * 64 + t * 32 + l31] = v;
            }
        }
        return;
    }
    float* __restrict__ Cg = p.C + bz * p.sC;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int col = j0 + wn * 128 + nt * 32 + l31;
        if (col >= p.Jc) continue;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < p.I) atomicAdd(Cg + tn_c_offset(p, row, 0, col), acc[mt][nt][r]);
            }
    }
    if (do_bias) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float v = bsum[t] + __shfl_xor(bsum[t], 32, 64);    // the two lane halves hold different m
            const int col = i0 + wm * 64 + t * 32 + l31;
            if (half == 0 && col < p.I) atomicAdd(p.colsumA + col, v);
        }
    }
#endif
}

// -------------------------------------------------------------------------------------------------
// 256 x 256 TN GEMM with the 8-phase main loop of gemm_nt_8phase_kernel (the DMA queue is never drained; seven half-tiles ahead; one
// counted vmcnt(6) per K tile): the weight gradients of the transformer's Linear layers, C[i][j] += sum_m A[m][i] B[m][j] with a long
// reduction per workgroup (>= 16 K tiles of 64 rows).  Operands stay in their natural [m][column] layout; a half-tile is 64 reduction
// rows x 128 columns (256-byte LDS rows, 16 KiB = two 1-KiB DMA pieces of 4 rows per wave), chunk c of row r at c ^ ((r & 3) << 2)
// -- the layout the transpose reads (ds_read_b64_tr_b16, as gemm_tn_wide_pipe_kernel) walk without bank conflicts.
// Slots, stream order, phases, RAW / WAR argument: gemm_nt_8phase_kernel's header (A0 / A1 = columns i0 .. + 127 / + 128 .. + 255 of A).
// Phase 0 issues 24 transpose reads (8 for B0 first); s_waitcnt lgkmcnt(15) -- the counter's maximum -- retires at least those 8
// before the barrier that lets the next phase re-stage B0's slot.  The DMA is inline assembly (the compiler would order every
// transpose read behind all LDS-DMA it knows of).  Epilogue as gemm_tn_wide_pipe_kernel (workspace partials or fp32 atomics).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void gemm_tn_8phase_kernel(TnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using T = bf16_t;
    constexpr int HROW = 256;                                // LDS row bytes of a half-tile: 128 bf16 columns
    constexpr int HTB = 64 * HROW;                           // 16 KiB
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;                 // 2 x 4 waves: 64 i-columns of both A halves x 32 j-columns of both B halves
    const int per_split = p.itiles * p.jtiles;
    int bx = xcd_remap(blockIdx.x, per_split * p.nsplit);
    const int split = bx / per_split;
    bx -= split * per_split;
    const int it = bx % p.itiles, jt = bx / p.itiles;
    const int i0 = it * 256, j0 = jt * 256;
    const int64_t bz = blockIdx.z;
    const T* Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    const int mbeg = split * p.m_per_split;
    const int mend = min(p.Mred, mbeg + p.m_per_split);
    const int nk = (mend - mbeg + 63) / 64;

    auto make_rsrc = [&](const T* base, int64_t bytes) {
        const unsigned long long a = (unsigned long long)base;
        int32x4 r;
        r.x = (int)(unsigned)a;
        r.y = (int)(unsigned)(a >> 32);
        r.z = (int)bytes;                                    // reads at or past this byte offset return zero
        r.w = 0x00020000;
        r.x = __builtin_amdgcn_readfirstlane(r.x);
        r.y = __builtin_amdgcn_readfirstlane(r.y);
        r.z = __builtin_amdgcn_readfirstlane(r.z);
        return r;
    };
    const int32x4 rsA = make_rsrc(Ag, (int64_t)mend * p.lda * 2), rsB = make_rsrc(Bg, (int64_t)mend * p.ldb * 2);
    // DMA piece e (0 / 1) of this wave in a half-tile: rows (2 wave + e) * 4 + (lane >> 4), chunk position lane & 15 <- source chunk pos ^ ((row & 3) << 2)
    int voA[2][2], voB[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int row = (2 * wave + e) * 4 + (lane >> 4);
            const int cg = (lane & 15) ^ ((row & 3) << 2);
            voA[i][e] = (int)(((int64_t)(mbeg + row) * p.lda + i0 + i * 128 + cg * 8) * 2);
            voB[i][e] = (int)(((int64_t)(mbeg + row) * p.ldb + j0 + i * 128 + cg * 8) * 2);
        }
    const int sstepA = (int)(64 * p.lda * 2), sstepB = (int)(64 * p.ldb * 2);      // bytes per K tile
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
    auto stage = [&](auto qtag, int kt, int slot) {          // half-tile q of the stream order (0: B0, 1: A0, 2: B1, 3: A1)
        constexpr int q = decltype(qtag)::value;
        const int ktc = min(kt, nk - 1);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const unsigned l = lds0 + (unsigned)(slot * HTB + (2 * wave + e) * 1024);
            const bool isA = (q & 1) != 0;
            const int so = __builtin_amdgcn_readfirstlane(ktc * (isA ? sstepA : sstepB));
            const int vo = isA ? voA[q >> 1][e] : voB[q >> 1][e];
            const int32x4 rs = isA ? rsA : rsB;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" : : "s"(l), "v"(vo), "s"(rs), "s"(so) : "memory");
        }
    };
    using Q0 = std::integral_constant<int, 0>;
    using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>;
    using Q3 = std::integral_constant<int, 3>;
    // fragment addressing (igemm_tn_tr_kernel's): a 16-lane group reads 4 rows x 16 columns per ds_read_b64_tr_b16
    const int g = lane >> 4, li = lane & 15;
    const int frow = 8 * (g >> 1) + (li >> 2);               // + 16 ks (+ 4 for the second read)
    const int fz = ((li >> 2) & 3) << 2;
    int offA[2], offB;
#pragma unroll
    for (int f = 0; f < 2; ++f) offA[f] = frow * HROW + (((wr * 8 + f * 4 + 2 * (g & 1) + ((li & 3) >> 1)) ^ fz) << 4) + (li & 1) * 8;
    offB = frow * HROW + (((wc * 4 + 2 * (g & 1) + ((li & 3) >> 1)) ^ fz) << 4) + (li & 1) * 8;
    const bool do_bias = p.colsumA != nullptr && jt == 0 && wc == 0;
    float bsum[2][2] = {{0.f, 0.f}, {0.f, 0.f}};

    f32x16 acc[2][2][2];                                    // [A half][B half][i tile of the quadrant]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][f][r] = 0.f;
    int par = 0;                                             // byte offset of the current K tile's slot group (0 / 4 * HTB)
    auto frag = [&](int off, int ks) -> bf16x8 {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(smem + off + (ks * 16) * HROW));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(smem + off + (ks * 16 + 4) * HROW));
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    bf16x8 a[2][4], b0[4], b1[4];
    auto read_a = [&](int i) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int f = 0; f < 2; ++f) a[f][ks] = frag(par + (2 * i + 1) * HTB + offA[f], ks);
    };
    auto read_b = [&](int j, bf16x8 (&b)[4]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) b[ks] = frag(par + 2 * j * HTB + offB, ks);
    };
    auto bias_of = [&](int i) {                              // column sums of A (dbias) from the fragments just read
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const uint4 u = __builtin_bit_cast(uint4, a[f][ks]);
                bsum[i][f] += (__uint_as_float(u.x << 16) + __uint_as_float(u.x & 0xffff0000u)) +
                              (__uint_as_float(u.y << 16) + __uint_as_float(u.y & 0xffff0000u)) +
                              (__uint_as_float(u.z << 16) + __uint_as_float(u.z & 0xffff0000u)) +
                              (__uint_as_float(u.w << 16) + __uint_as_float(u.w & 0xffff0000u));
            }
    };
    auto mfma8 = [&](int i, int j, bf16x8 (&b)[4]) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int f = 0; f < 2; ++f)
                acc[i][j][f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f][ks], b[ks], acc[i][j][f], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto bar = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    if (nk > 0) {
        stage(Q0{}, 0, 0);
        stage(Q1{}, 0, 1);
        stage(Q2{}, 0, 2);
        stage(Q3{}, 0, 3);
        stage(Q0{}, 1, 4);
        stage(Q1{}, 1, 5);
        stage(Q2{}, 1, 6);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        bar();
        if (wr == 1) bar();                                   // the second wave group runs one barrier behind
#pragma unroll 1
        for (int t = 0; t < nk; ++t) {
            const int cur = (t & 1) * 4, nxt = cur ^ 4;
            // ---- phase 0: quadrant (A0, B0) ----
            read_b(0, b0);
            __builtin_amdgcn_sched_barrier(0);
            read_a(0);
            __builtin_amdgcn_sched_barrier(0);
            stage(Q3{}, t + 1, nxt + 3);
            asm volatile("s_waitcnt lgkmcnt(15)" ::: "memory");   // >= 9 of the 24 reads have returned, the 8 of B0 among them
            bar();
            if (do_bias) bias_of(0);
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
            if (do_bias) bias_of(1);
            mfma8(1, 1, b1);
            bar();
            // ---- phase 3: quadrant (A1, B0) ----
            stage(Q2{}, t + 2, cur + 2);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // all but the three youngest half-tiles: K tile t + 1 is complete
            bar();
            mfma8(1, 0, b0);
            bar();
            par ^= 4 * HTB;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wr == 0) bar();
    }

    const int l31 = lane & 31, half = lane >> 5;
    if (p.ws != nullptr) {
        float* tile = p.ws + ((int64_t)split * per_split + it + (int64_t)jt * p.itiles) * 65536;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        tile[(i * 128 + wr * 64 + f * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 256 + j * 128 + wc * 32 + l31] = acc[i][j][f][r];
        if (do_bias) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const float v = bsum[i][f] + __shfl_xor(bsum[i][f], 32, 64);
                    if (half == 0) p.ws_bias[((int64_t)split * p.itiles + it) * 256 + i * 128 + wr * 64 + f * 32 + l31] = v;
                }
        }
        return;
    }
    float* __restrict__ Cg = p.C + bz * p.sC;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = j0 + j * 128 + wc * 32 + l31;
        if (col >= p.Jc) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i0 + i * 128 + wr * 64 + f * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (row < p.I) atomicAdd(Cg + tn_c_offset(p, row, 0, col), acc[i][j][f][r]);
                }
    }
    if (do_bias) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const float v = bsum[i][f] + __shfl_xor(bsum[i][f], 32, 64);    // the two lane halves hold different m
                const int col = i0 + i * 128 + wr * 64 + f * 32 + l31;
                if (half == 0 && col < p.I) atomicAdd(p.colsumA + col, v);
            }
    }
#endif
}

// C[i][j] += sum over the splits of the workspace partials (one writer per element: plain read-modify-write, deterministic order)
__global__ __launch_bounds__(256) void gemm_tn_wide_reduce_kernel(TnParams p) {
    const int ntile = p.itiles * p.jtiles;
    const int64_t total = (int64_t)ntile * 65536;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int wi = (int)(e >> 16), q = (int)(e & 65535);
        const int row = (wi % p.itiles) * 256 + (q >> 8), col = (wi / p.itiles) * 256 + (q & 255);
        if (row >= p.I || col >= p.Jc) continue;
        const float* src = p.ws + (int64_t)wi * 65536 + q;
        const int64_t sstride = (int64_t)ntile * 65536;
        float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // eight loads in flight per thread
        int sidx = 0;
        for (; sidx + 8 <= p.nsplit; sidx += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) s8[u] += src[(sidx + u) * sstride];
        }
        for (; sidx < p.nsplit; ++sidx) s8[0] += src[sidx * sstride];
        p.C[tn_c_offset(p, row, 0, col)] += ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    }
    if (p.colsumA != nullptr) {
        for (int e = blockIdx.x * 256 + threadIdx.x; e < p.itiles * 256; e += gridDim.x * 256) {
            if (e >= p.I) continue;
            float sum = 0.f;
            for (int sidx = 0; sidx < p.nsplit; ++sidx) sum += p.ws_bias[((int64_t)sidx * p.itiles + (e >> 8)) * 256 + (e & 255)];
            p.colsumA[e] += sum;
        }
    }
}

// one wave per output element C[i][tap*J + j]; lanes stride the reduction dimension
template <typename T>
__global__ void naive_tn_kernel(TnParams p) {
    const int64_t bz = blockIdx.z;
    const T* Ag = reinterpret_cast<const T*>(p.A) + bz * p.sA;
    const T* Bg = reinterpret_cast<const T*>(p.B) + bz * p.sB;
    float* Cg = p.C + bz * p.sC;
    const int lane = threadIdx.x & 63;
    const int64_t nout = (int64_t)p.I * p.taps * p.J;
    const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / 64;
    for (int64_t e = wid; e < nout + (p.colsumA ? p.I : 0); e += nw) {
        float acc = 0.f;
        if (e >= nout) {   // column sums of A
            const int i = (int)(e - nout);
            for (int m = lane; m < p.Mred; m += 64) acc += ElemIO<T>::load(Ag + (int64_t)m * p.lda + i);
            acc = wave_sum(acc);
            if (lane == 0) atomicAdd(p.colsumA + i, acc);
            continue;
        }
        const int i = (int)(e / ((int64_t)p.taps * p.J));
        const int rest = (int)(e % ((int64_t)p.taps * p.J));
        const int tap = rest / p.J, j = rest % p.J;
        const int kh = tap / p.KW, kw = tap % p.KW;
        const int hw = p.DH * p.DW;
        for (int m = lane; m < p.Mred; m += 64) {
            float bv;
            if (!p.conv) {
                bv = ElemIO<T>::load(Bg + (int64_t)m * p.ldb + j);
            } else {
                const int n = m / hw, rem = m % hw, y = rem / p.DW, x = rem % p.DW;
                const int ih = y * p.stride - p.pad_t + kh, iw = x * p.stride - p.pad_l + kw;
                if ((unsigned)ih >= (unsigned)p.LH || (unsigned)iw >= (unsigned)p.LW) continue;
                bv = ElemIO<T>::load(Bg + (((int64_t)n * p.SH + (ih >> p.up)) * p.SW + (iw >> p.up)) * p.ldb + j);
            }
            acc = fmaf(ElemIO<T>::load(Ag + (int64_t)m * p.lda + i), bv, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0 && j < p.Jc) atomicAdd(Cg + tn_c_offset(p, i, tap, j), acc);
    }
}

// deterministic mode: C[e] += sum over the splits' partial slices, in split order (one thread per element: a fixed summation order)
__global__ __launch_bounds__(256) void tn_det_fold_kernel(float* __restrict__ C, const float* __restrict__ ws, int nsplit, int64_t stride,
                                                          int64_t n, float* __restrict__ colsum, const float* __restrict__ ws_bias, int I) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) {
        float acc = 0.f;
        for (int sidx = 0; sidx < nsplit; ++sidx) acc += ws[(int64_t)sidx * stride + e];
        C[e] += acc;
    }
    if (colsum != nullptr && e < I) {
        float acc = 0.f;
        for (int sidx = 0; sidx < nsplit; ++sidx) acc += ws_bias[(int64_t)sidx * I + e];
        colsum[e] += acc;
    }
}

// deterministic partials for the split TN kernels: C must be ONE contiguous span of `span` floats (a parameter's gradient is)
static bool tn_det_setup(TnParams& p, int64_t batch, hipStream_t s, int64_t* span_out) {
    const int64_t row_w = (int64_t)p.taps * p.Jc;
    if (batch != 1 || p.nsplit <= 1 || (!p.c_oihw && p.ldc != row_w)) return false;
    const int64_t span = (int64_t)p.I * row_w;
    int64_t ws_bytes = 0;
    char* wsp = (char*)dvq_workspace_stream(s, &ws_bytes);
    const int64_t need = ((int64_t)p.nsplit * span + (int64_t)p.nsplit * p.I) * 4;
    if (wsp == nullptr || ws_bytes < need) return false;
    p.dws = (float*)wsp;
    p.dws_stride = span;
    p.dws_bias = p.colsumA != nullptr ? (float*)wsp + (int64_t)p.nsplit * span : nullptr;
    *span_out = span;
    return true;
}
static void tn_det_fold(const TnParams& p, int64_t span, hipStream_t s) {
    const int64_t n = span > p.I ? span : p.I;
    tn_det_fold_kernel<<<dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s>>>(p.C, p.dws, p.nsplit, p.dws_stride, span, p.dws_bias ? p.colsumA : nullptr,
                                                                           p.dws_bias, p.I);
}

// large plain weight-gradient GEMMs (bf16): 256 x 256 tiles, pipelined main loop; ~one resident workgroup per CU.
// 1 x 1 weight gradients run on the patch kernel too, not on this one: 65536 x 256 x 256
// 31 against 52 us, 16384 x 512 x 512 30 against 40 us -- a 256 x 256 tile leaves 64 workgroups for the whole chip
bool tn_wide_ok(const TnParams& p) {
    return !p.conv && p.taps == 1 && p.I >= 256 && p.J >= 256 && p.Mred >= 1024 &&
           p.I % 8 == 0 && p.J % 8 == 0 && (int64_t)p.Mred * p.lda < (1ll << 30) && (int64_t)p.Mred * p.ldb < (1ll << 30) &&
           (p.sA * 2) % 4 == 0 && (p.sB * 2) % 4 == 0;
}

// eight_phase: gemm_tn_8phase_kernel (DMA queue never drained; batch strides must be multiples of 16 bytes), else gemm_tn_wide_pipe_kernel
int launch_tn_wide(TnParams p, int64_t batch, bool det, bool eight_phase, hipStream_t s) {
    constexpr int BK = Vec<bf16_t>::BK;
    p.itiles = (int)cdiv64(p.I, 256);
    p.jtiles = (int)cdiv64(p.J, 256);
    const int64_t wtiles = (int64_t)p.itiles * p.jtiles * batch;
    // workgroups a wide TN product aims at.  Round 5: 128, not one per CU -- these weight gradients run on the side stream beside
    // the input-gradient GEMMs (layers.Linear.bwd), so half a chip's worth of workgroups is what they get anyway, and half the
    // splits mean half the partials to write and fold: StackGPT p6c18 step 79.9 -> 77.9 ms (64: 81.3 ms; same-box A/B,
    // profiles/r05_stage2_ab.txt).
    constexpr int wide_wgs = 128;
    int64_t wsplits = wtiles >= wide_wgs ? 1 : wide_wgs / wtiles;
    // >= 16 stages per workgroup: prologue, partial-tile store and fold amortised (8 / 4 / 32 measured slower on the 1 x 1
    // weight gradients: 60 / 95 / 66 against 52 us at 65536 x 256 x 256)
    const int64_t wmax = cdiv64(p.Mred, 16 * BK);
    if (wsplits > wmax) wsplits = wmax;
    const int64_t wmps = cdiv64(cdiv64(p.Mred, wsplits), BK) * BK;
    p.m_per_split = (int)wmps;
    p.nsplit = (int)cdiv64(p.Mred, wmps);
    int64_t ws_bytes = 0;
    char* wsp = (char*)dvq_workspace_stream(s, &ws_bytes);
    const int64_t need = (int64_t)p.nsplit * wtiles * 65536 * 4 + (int64_t)p.nsplit * p.itiles * 256 * 4;
    if (wsp != nullptr && ws_bytes >= need && (p.nsplit > 2 || (det && p.nsplit > 1)) && batch == 1) {     // many splits per tile: partials + fold, no atomics
        p.ws = (float*)wsp;
        p.ws_bias = (float*)(wsp + (int64_t)p.nsplit * wtiles * 65536 * 4);
    } else if (det && p.nsplit > 1) {            // no scratch for the partials: one workgroup per tile walks the whole reduction
        p.m_per_split = (int)(cdiv64(p.Mred, BK) * BK);
        p.nsplit = 1;
    }
    if (p.ws == nullptr && p.nsplit > 1) dvq_note_unordered();      // two splits (or a batched product without scratch): fp32 atomics into C
    if (eight_phase) {
        dvq_note_kernel("gemm_tn_8phase_kernel");
        dvq_ensure_dynamic_lds((const void*)gemm_tn_8phase_kernel, 8 * 64 * 256);
        gemm_tn_8phase_kernel<<<dim3((unsigned)(p.itiles * p.jtiles * p.nsplit), 1, (unsigned)batch), dim3(512), 8 * 64 * 256, s>>>(p);
        DVQ_CHECK_LAUNCH("gemm_tn_8phase");
    } else {
        dvq_note_kernel("gemm_tn_wide_pipe_kernel");
        dvq_ensure_dynamic_lds((const void*)gemm_tn_wide_pipe_kernel, 2 * WTSTG);
        gemm_tn_wide_pipe_kernel<<<dim3((unsigned)(p.itiles * p.jtiles * p.nsplit), 1, (unsigned)batch), dim3(512), 2 * WTSTG, s>>>(p);
        DVQ_CHECK_LAUNCH("gemm_tn_wide_pipe");
    }
    if (p.ws != nullptr) {
        gemm_tn_wide_reduce_kernel<<<dim3((unsigned)(wtiles * 256)), dim3(256), 0, s>>>(p);
        DVQ_CHECK_LAUNCH("gemm_tn_wide_reduce");
    }
    return DVQ_OK;
}

// 8 x 8 output-pixel patches as reduction stages (conv_tn_patch_kernel, bf16, batch 1, not the thin J == 8 shapes)
bool tn_patch_ok(const TnParams& p) {
    return p.conv && !p.thin && p.I % 8 == 0 && p.J % 8 == 0 &&
           p.pad_t <= 8 && p.pad_l <= 8 && p.Mred % (p.DH * p.DW) == 0 &&
           (int64_t)(8 * p.stride + p.taps / p.KW + 10) * p.SW * p.ldb * 2 < (1ll << 30) && (int64_t)8 * p.DW * p.lda * 2 < (1ll << 30);
}

// split over patch ranges
int launch_tn_patch(TnParams p, int64_t batch, bool det, hipStream_t s) {
    const int64_t PH = cdiv64(p.DH, 8), PW = cdiv64(p.DW, 8);
    const int64_t npatch = (p.Mred / ((int64_t)p.DH * p.DW)) * PH * PW;
    const int64_t ptiles = (int64_t)p.itiles * p.jtiles * p.taps;
    int64_t psplits = 512 / ptiles;          // workgroups the patch kernel aims at (sweep: 128 / 256 / 512 / 1024, profiles/)
    if (psplits > npatch / 16) psplits = npatch / 16;       // >= 16 stages per workgroup: the 64-KiB atomic flush amortised
    if (psplits < 1) psplits = 1;
    int64_t pps = cdiv64(npatch, psplits);
    p.m_per_split = (int)pps;
    p.nsplit = (int)cdiv64(npatch, pps);
    int64_t dspan = 0;
    const bool dfold = det && p.nsplit > 1 && tn_det_setup(p, batch, s, &dspan);      // partials + fold in split order
    if (det && p.nsplit > 1 && !dfold) {                                             // no scratch / strided C: unsplit
        p.m_per_split = (int)npatch;
        p.nsplit = 1;
    }
    if (p.nsplit > 1 && !dfold) dvq_note_unordered();
    dvq_note_kernel("conv_tn_patch_kernel");
    dvq_ensure_dynamic_lds((const void*)conv_tn_patch_kernel, 2 * TSTAGEB);
    conv_tn_patch_kernel<<<dim3((unsigned)(ptiles * p.nsplit)), dim3(256), 2 * TSTAGEB, s>>>(p);
    DVQ_CHECK_LAUNCH("conv_tn_patch");
    if (dfold) {
        tn_det_fold(p, dspan, s);
        DVQ_CHECK_LAUNCH("tn_det_fold");
    }
    return DVQ_OK;
}

// 128 x 128 tiles split along the reduction: the LDS-DMA + transpose-read kernel (bf16, tr) or the register-staged igemm_tn_kernel
template <typename T>
int launch_tn_tiles(TnParams p, int64_t batch, bool tr, bool det, hipStream_t s) {
    constexpr int BK = Vec<T>::BK;
    const int tapblk = p.thin ? 1 : p.taps;
    const int64_t tiles = (int64_t)p.itiles * p.jtiles * tapblk * batch;
    // 512 resident workgroups (2 per CU): aim at two full rounds, never slightly more than a round
    // (thin: every workgroup ends with I x taps x 8 atomics on one small tile -- one round of 256 is enough)
    int64_t splits = (p.thin ? 256 : 1024) / tiles;
    const int64_t max_splits = cdiv64(p.Mred, 4 * BK);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    int64_t mps = cdiv64(cdiv64(p.Mred, splits), BK) * BK;
    splits = cdiv64(p.Mred, mps);
    p.m_per_split = (int)mps;
    p.nsplit = (int)splits;
    dim3 grid((unsigned)(p.itiles * p.jtiles * tapblk * splits), 1, (unsigned)batch);
    int64_t gspan = 0;
    bool gfold = false;
    if (det && p.nsplit > 1) {
        gfold = tn_det_setup(p, batch, s, &gspan);                // partials + fold in split order
        if (!gfold) {                                                                    // batched / strided C / no scratch: unsplit
            p.m_per_split = (int)(cdiv64(p.Mred, BK) * BK);
            p.nsplit = 1;
            grid = dim3((unsigned)(p.itiles * p.jtiles * tapblk), 1, (unsigned)batch);
        }
    }
    // fp32 atomics from several splits per element -- and, on the register-staged kernel, from the row blocks of ONE workgroup per column sum
    if (p.nsplit > 1 && !gfold) dvq_note_unordered();
    else if (!tr && !det && p.colsumA != nullptr) dvq_note_unordered();
    dvq_note_kernel(tr ? "igemm_tn_tr_kernel" : "igemm_tn_kernel");
    if (tr) {
        if (p.conv) {
            dvq_ensure_dynamic_lds((const void*)igemm_tn_tr_kernel<true>, 2 * TSTAGEB);
            igemm_tn_tr_kernel<true><<<grid, dim3(256), 2 * TSTAGEB, s>>>(p);
        } else {
            dvq_ensure_dynamic_lds((const void*)igemm_tn_tr_kernel<false>, 2 * TSTAGEB);
            igemm_tn_tr_kernel<false><<<grid, dim3(256), 2 * TSTAGEB, s>>>(p);
        }
    } else if (sizeof(T) == 4 && p.split3) {          // fp32x3
        constexpr bool F32 = sizeof(T) == 4;
        if (p.conv) {
            dvq_ensure_dynamic_lds((const void*)igemm_tn_kernel<T, true, F32>, 2 * GSTAGEB);
            igemm_tn_kernel<T, true, F32><<<grid, dim3(256), 2 * GSTAGEB, s>>>(p);
        } else {
            dvq_ensure_dynamic_lds((const void*)igemm_tn_kernel<T, false, F32>, 2 * GSTAGEB);
            igemm_tn_kernel<T, false, F32><<<grid, dim3(256), 2 * GSTAGEB, s>>>(p);
        }
    } else if (p.conv) {
        dvq_ensure_dynamic_lds((const void*)igemm_tn_kernel<T, true>, 2 * GSTAGEB);
        igemm_tn_kernel<T, true><<<grid, dim3(256), 2 * GSTAGEB, s>>>(p);
    } else {
        dvq_ensure_dynamic_lds((const void*)igemm_tn_kernel<T, false>, 2 * GSTAGEB);
        igemm_tn_kernel<T, false><<<grid, dim3(256), 2 * GSTAGEB, s>>>(p);
    }
    DVQ_CHECK_LAUNCH("igemm_tn");
    if (gfold) {
        tn_det_fold(p, gspan, s);
        DVQ_CHECK_LAUNCH("tn_det_fold");
    }
    return DVQ_OK;
}

template <typename T>
int launch_tn_naive(TnParams p, int64_t batch, hipStream_t s) {
    int64_t nout = (int64_t)p.I * p.taps * p.J + (p.colsumA ? p.I : 0);
    unsigned blocks = (unsigned)(cdiv64(nout, 4) < 8192 ? cdiv64(nout, 4) : 8192);
    dvq_note_kernel("naive_tn_kernel");
    naive_tn_kernel<T><<<dim3(blocks, 1, (unsigned)batch), dim3(256), 0, s>>>(p);
    DVQ_CHECK_LAUNCH("naive_tn");
    return DVQ_OK;
}

}  // namespace

// Priority order: naive (DVQ_IMPL_NAIVE, or the automatic choice on an unaligned / short reduction), wide 8-phase / wide pipe, patch stages,
// transpose-read, register-staged.  Every code from DVQ_IMPL_MFMA up takes an MFMA kernel; all but the NT-only preferred codes
// DVQ_IMPL_WIDE .. DVQ_IMPL_WIDE_PIPE_192 return DVQ_ESHAPE without the vector alignment.
template <typename T>
int launch_tn(TnParams p, int64_t batch, int impl, hipStream_t s) {
    constexpr int VN = Vec<T>::N;
    p.split3 = sizeof(T) == 4 && dvq_fp32_split() != 0;
    const bool mfma_ok = p.lda % VN == 0 && p.ldb % VN == 0 && p.sA % VN == 0 && p.sB % VN == 0;
    DVQ_REQUIRE(mfma_ok || impl < DVQ_IMPL_MFMA || (impl_preferred(impl) && impl != DVQ_IMPL_8PHASE), DVQ_ESHAPE,
                "igemm_tn: MFMA path needs lda, ldb multiples of %d", VN);
    const bool use_mfma = impl >= DVQ_IMPL_MFMA || (impl == DVQ_IMPL_AUTO && mfma_ok && (int64_t)p.Mred >= 256);
    if (!use_mfma) return launch_tn_naive<T>(p, batch, s);
    // the transpose-read kernel takes every bf16 product except under DVQ_IMPL_REGSTAGE
    const bool tr = sizeof(T) == 2 && impl != DVQ_IMPL_REGSTAGE;
    p.itiles = (int)cdiv64(p.I, TILE);
    p.jtiles = (int)cdiv64(p.J, TILE);
    p.thin = (p.conv && tr && p.J == 8 && p.taps <= 16 && p.taps > 1) ? 1 : 0;
    // opt-in: no fp32 atomics from more than one writer per output element, for both operand types: every split kernel stores
    // partials for tn_det_fold_kernel, or runs unsplit where C is batched / strided or no scratch is registered
    const bool det = dvq_deterministic() != 0;
    p.det = det ? 1 : 0;
    if constexpr (sizeof(T) == 2) {
        // DVQ_IMPL_WIDE_PIPE asks for the per-stage-drain kernel (tests) in place of the 8-phase one
        if ((impl == DVQ_IMPL_AUTO || impl == DVQ_IMPL_WIDE_PIPE) && tn_wide_ok(p))
            return launch_tn_wide(p, batch, det, impl == DVQ_IMPL_AUTO && (p.sA * 2) % 16 == 0 && (p.sB * 2) % 16 == 0, s);
        if (impl == DVQ_IMPL_AUTO && batch == 1 && tn_patch_ok(p)) return launch_tn_patch(p, batch, det, s);
    }
    return launch_tn_tiles<T>(p, batch, tr, det, s);
}

template int launch_tn<float>(TnParams, int64_t, int, hipStream_t);
template int launch_tn<bf16_t>(TnParams, int64_t, int, hipStream_t);

}  // namespace igemm
