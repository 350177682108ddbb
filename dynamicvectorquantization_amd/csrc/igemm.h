// Host-side contract between the conv / GEMM front end (igemm.hip) and the two kernel files: the parameter blocks, and the one
// dispatcher each side exports.  igemm_nt.hip defines launch_nt / launch_nt_skinny, igemm_tn.hip defines launch_tn; kernels are launched
// only from the file that holds them.  No device code here.
#pragma once
#include "dvq_common.h"

namespace igemm {

enum { MODE_FWD = 0, MODE_TCONV = 1, MODE_GEMM = 2 };

struct NtParams {
    const void* A;
    const void* B;
    void* C;
    const void* R;       // residual (same layout as C) or null
    const float* bias;
    int mode;
    int M, Ncols, Ktot;  // GEMM dims (elements)
    int64_t lda;         // GEMM: A row stride; conv: Cs (source channels)
    int64_t ldb, ldc;
    int SH, SW;          // stored source grid
    int LH, LW;          // logical bounds (FWD: H,W after upsample; TCONV: OH,OW)
    int DH, DW;          // destination pixel grid (rows of the GEMM)
    int KW, stride, pad_t, pad_l, up;
    float alpha;
    int bias_mode;       // 0 none, 1 per column, 2 per row
    int64_t sA, sB, sC;  // batch strides
    int gm, gn;          // tile grid (M tiles x N tiles); the launch grid is 1-D over gm*gn, XCD-remapped
    float act_slope;     // output activation v > 0 ? v : act_slope * v (1: none, 0: ReLU, 0.2: LeakyReLU), applied last
    int res_mask;        // 1: R gates instead of adds: v *= (R > 0 ? 1 : mask_slope) (ReLU / LeakyReLU backward)
    float mask_slope;
    int par;             // TCONV, stride 2: GEMM rows are grouped by output-pixel parity class (y & 1, x & 1); a tile then
    int par_tiles;       //   contracts only over the taps that reach its class (1/4 of a 4x4 kernel) -- M tiles per class
    int split3;          // fp32 operands: 1 = two bf16 planes + three bf16 MFMA passes (dvq_set_fp32_split), 0 = v_mfma_f32_32x32x2_f32
};

struct TnParams {
    const void* A;   // [Mred][lda]           (wgrad: dy, lda = Cout)
    const void* B;   // GEMM: [Mred][ldb]; conv: gathered from x (Cs = ldb)
    float* C;
    float* colsumA;  // optional: colsumA[i] += sum_m A[m][i]  (dbias), done by tap-0 / jtile-0 blocks
    int conv;        // 0 plain, 1 gather B rows through the FWD conv geometry
    int Mred, I, J;
    int64_t lda, ldb, ldc;
    int taps, jtiles, itiles;
    int SH, SW, LH, LW, DH, DW, KW, stride, pad_t, pad_l, up;
    int m_per_split, nsplit;
    int c_oihw;      // 1: C is laid out [I][Jc][taps] (element (i, tap, j) at (i*Jc + j)*taps + tap); 0: [I][taps][Jc] with row stride ldc
    int Jc;          // columns per tap of C (<= J; smaller when the operand channels are padded)
    int64_t sA, sB, sC;
    int batch_in_z;
    float* ws;       // wide pipelined kernel: split partials [nsplit][tiles][256][256] fp32 (+ ws_bias [nsplit][itiles][256]) in the
    float* ws_bias;  //   registered workspace, folded by gemm_tn_wide_reduce_kernel; null -> fp32 atomics straight into C
    int thin;        // conv, J == 8 (image-channel inputs): the B tile's 16 chunks are the TAPS (column = tap * 8 + channel), one
                     //   workgroup accumulates every tap instead of a 1/16-full tile per tap
    float* dws;      // deterministic mode (dvq_set_deterministic): split s STORES its partial of C at dws + s * dws_stride (same element
    int64_t dws_stride;   //   offsets as C, which must be one contiguous span) and its bias partial at dws_bias + s * I; tn_det_fold_kernel
    float* dws_bias;      //   adds the slices to C / colsumA in split order.  null: fp32 atomics straight into C (default)
    int split3;           // fp32 operands: two bf16 planes + three bf16 MFMA passes (dvq_set_fp32_split)
    int det;              // deterministic mode: igemm_tn_kernel adds the column sums of a workgroup's row blocks in LDS, in block order,
                          //   instead of with one atomic per thread (several threads of ONE workgroup own the same column)
};

// preferred impl codes (include/dvq_hip.h) ask for a kernel and take the automatic choice on a shape that kernel does not run
inline bool impl_preferred(int impl) {
    return impl == DVQ_IMPL_WIDE || impl == DVQ_IMPL_WIDE_PIPE || impl == DVQ_IMPL_WIDE_PIPE_4WAVE || impl == DVQ_IMPL_WIDE_PIPE_192 ||
           impl == DVQ_IMPL_8PHASE;
}

// try the kernels of one side in priority order (explicitly instantiated for float and bf16_t)
template <typename T>
int launch_nt(NtParams p, int64_t batch, int impl, hipStream_t s);
template <typename T>
int launch_tn(TnParams p, int64_t batch, int impl, hipStream_t s);
// gemm_nt_skinny_kernel (bf16, M <= 32, batch 1): the caller checks eligibility
int launch_nt_skinny(const NtParams& p, hipStream_t s);

}  // namespace igemm
