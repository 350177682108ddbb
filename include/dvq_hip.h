/*
 * dvq_hip.h -- C ABI of libdvq_hip.so: the MI355X (gfx950) kernels of the DQ-VAE hot path.
 *
 * The reference (CrossmodalGroup/DynamicVectorQuantization) has no FFI of its own: its operator
 * boundary is the Python `target:`/`params:` plugin API (utils/utils.py:41-51) and every kernel is an
 * ATen call.  This header is the boundary a maintainer binds with ctypes from those Python modules
 * (see INTEGRATION.md); each entry point cites the reference call site it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (incl. workspaces); the library allocates
 *     nothing, launches only on `stream`, never synchronises.  Process-wide state is limited to, and listed here:
 *     the scratch registration of dvq_set_workspace() (one caller-owned buffer per process, i.e. per rank / device, cut into
 *     eight equal slots that are handed to the streams using them; a slot requested during stream capture stays with its
 *     stream until dvq_workspace_release(); set it once before the first call that uses it; calls that find no slot or a slot
 *     too small fall back to atomics) and caches of one-off hipFuncSetAttribute calls.
 *     dvq_probe_mfma_rate (diagnostics) and dvq_decode_stack_status are the entry points that allocate or synchronise;
 *     no vendor BLAS / DNN library is linked or loaded: every product is a kernel of this library;
 *   - every entry point issues KERNEL launches only (no memset / memcpy nodes), so a sequence of calls can be recorded by
 *     HIP stream capture after its first eager execution and replayed (the training step and the sampler do);
 *   - activations are NHWC ("pixel-major"): element (n,h,w,c) at ((n*H+h)*W+w)*C+c;
 *   - conv weights are OHWI: element (co,kh,kw,ci) at ((co*KH+kh)*KW+kw)*Cin+ci
 *     (= torch.channels_last storage of the reference's [Cout,Cin,KH,KW] parameter);
 *   - `dtype` is DVQ_F32 or DVQ_BF16 and applies to activations and packed weights; statistics,
 *     losses, optimizer state and codebooks are always fp32;
 *   - return value 0 on success, negative DVQ_E* otherwise; dvq_last_error() gives a thread-local
 *     message.  Nothing is thrown across the boundary.
 */
#ifndef DVQ_HIP_H
#define DVQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dvq_stream_t; /* hipStream_t */
typedef void* dvq_cmdlist_t; /* launch list built from a captured hipGraph_t (dvq_cmdlist_create) */

enum { DVQ_F32 = 0, DVQ_BF16 = 1 };
enum { DVQ_OK = 0, DVQ_EINVAL = -1, DVQ_ESHAPE = -2, DVQ_EARCH = -3, DVQ_ELAUNCH = -4, DVQ_EWORKSPACE = -5 };

const char* dvq_last_error(void);
/* Kernel family the calling thread's last dvq_conv2d_* / dvq_gemm_* call landed on: the `__global__` name of its primary kernel as
 * written in csrc ("conv3x3_halo_kernel", "conv_nt_pipe_kernel", ...; no template arguments, no fold / reduce / transpose helpers), noted
 * at the dispatch branch that launches it.  "" when nothing was noted (those entry points clear it first).  For timing labels.
 * Two values are ROUTE labels, not `__global__` names: "conv_x3_halo" and "conv_wgrad_x3_planes", the fp32x3 launch-level schemes of
 * dvq_conv2d_scratch_bytes (plane passes + the bf16 kernels behind them). */
const char* dvq_last_kernel(void);
int dvq_version(void);     /* 124 (additions since, no signature changed, no symbol removed: dvq_recon_cells (+ _workspace_bytes), dvq_nll_cell_sums: per-cell
                            * error and likelihood maps, docs/design/30-cell-maps.md; dvq_feat_moments, dvq_pair_scan (+ _workspace_bytes): sample-set
                            * metrics, docs/design/32-sample-set-metrics.md): dvq_conv2d_fwd / _dgrad / _wgrad take (scratch, scratch_bytes) and route the fp32x3 launch-level schemes themselves;
                            * dvq_conv2d_scratch_bytes replaces dvq_conv3x3_x3_ok, dvq_conv3x3_x3_scratch_bytes and dvq_conv2d_wgrad_x3_scratch_bytes;
                            * dvq_conv2d_fwd_x3, dvq_conv2d_dgrad_x3 and dvq_conv2d_wgrad_oihw_x3 are gone;
                            * 123: struct dvq_token_rule, DVQ_TOKEN_RULE_MAXV: dvq_sample_constrained, dvq_sample_guided, dvq_codec_tables, dvq_codec_record and
                            * dvq_codec_decode_step take the constraint rule as one block instead of nine loose arguments;
                            * 122: dvq_attn_causal_fwd / _bwd take the row pitch ldqkv (dvq_attn_causal_fwd_ld / _bwd_ld are gone); dvq_attn_causal_scratch_bytes
                            * is what the kernels that run need (0 forward at head sizes 128 / 256: NULL scratch); dvq_attn_full_scratch_bytes is gone;
                            * 121: dvq_halo_trace_read is gone (the timing experiments and the persistent 3x3 kernel left the sources: one library);
                            * 120: dvq_conv3x3_subpixel_ok, dvq_conv_desc.upsample == 2, bit 9 of the weight packs' dtype (nearest x2 + 3x3 convolutions
                            * as four 2x2 sub-pixel convolutions, forward and input gradient);
                            * 119: dvq_scalar_push (+ dvq_scalar_push_state_bytes), dvq_codebook_health (training metric logs);
                            * 118: dvq_unordered_launches; dvq_set_deterministic orders every floating-point reduction of a training step;
                            * 117: DVQ_IMPL_* names for the impl codes; one entry per convolution / GEMM pass (dvq_conv2d_fwd, _dgrad, _wgrad, dvq_gemm_tn
                            * take the arguments of their former _ex / _act / _mask / _oihw / _colsum variants; dvq_gemm_nt_res is gone);
                            * 116: dvq_grain_overlay, dvq_grain_lines, dvq_image_grid_u8 (+ dvq_image_grid_shape, dvq_imagelog_workspace_bytes):
                            * training-time image logging;
                            * 115: dvq_vq_sample_argmax (+ dvq_vq_trained_prepare), dvq_vq_gumbel_noise, dvq_vq_codebook_grad, dvq_vq_mask_ratio,
                            * dvq_vq_rownorm / _ortho_sumsq / _rownorm_bwd (gradient-trained codebook: Gumbel search, codebook gradient, orthogonality term);
                            * 114: dvq_tokens_pack, dvq_tokens_unpack (token shards: stored code maps <-> stage-2 streams);
                            * 113: dvq_last_kernel (kernel family of a conv call), dvq_attn_causal_ok / dvq_attn_full_ok / dvq_decode_stack_ok;
                            * 112: dvq_token_nll, dvq_nll_segment_sums (teacher-forced likelihood scoring);
                            * 111: dvq_sample_guided (classifier-free-guided constrained draw), dvq_label_dropout (null-label dropout);
                            * 110: dvq_recon_metrics (+ _workspace_bytes), dvq_code_histogram (reconstruction evaluation);
                            * 109: round 5 (dvq_conv2d_fwd_x3 / dvq_conv2d_dgrad_x3: fp32x3 3 x 3 convolutions on the halo kernel, fp32 output);
                            * 108: round 5 (dvq_split_bf16_planes, dvq_conv2d_wgrad_oihw_x3: fp32x3 weight gradients on the bf16 kernels);
                            * 107: round 5 (dvq_lpips_head_drop; probe modes compiled out of the product library);
                            * 106: round 4 (launch lists dvq_cmdlist_*, dvq_add_uniform, dvq_decode_stack_status + 64 sequences, drop_mask argument
                            * of dvq_attn_causal_fwd / bwd + dvq_attn_causal_mask_bytes, dvq_layernorm_bwd_res, dvq_dropout_add, eight
                            * workspace slots + dvq_workspace_release, vq_argmin workspace report slots);
                            * 105: round 3 (fused constrained sampler, GroupNorm-backward partials argument,
                            * no vendor-library entry points; + dvq_decode_stack, dvq_gemm_tn_colsum) */
/* 0 if the current HIP device is gfx950, DVQ_EARCH otherwise */
int dvq_check_device(void);
/* Deterministic summation (opt-in; default: environment DVQ_DETERMINISTIC=1, else off).  On: no kernel of a training step lets a
 * floating-point result depend on arrival order, neither across workgroups in global memory nor across waves in LDS.  Every
 * reduction takes one of two forms: per-split partials in the registered workspace (dvq_set_workspace) + a fold in split order with one
 * owner per output element, or one owner that walks its inputs in index order.  Covered: the weight gradients of every TN / halo
 * family for bf16, fp32 and fp32x3 operands with their column sums (bias gradients), dvq_sum_batch, the GroupNorm / BatchNorm
 * statistics and backward sums, the statistics epilogue of the halo convolution, the LayerNorm backward, the embedding gradient, the
 * cross-entropy / L1 / commitment / LPIPS loss sums, the VQ-EMA statistics and the trained-codebook gradient.  Without a workspace
 * (or with one too small) a call launches UNSPLIT or returns DVQ_EWORKSPACE / DVQ_ESHAPE -- never the atomic form.  Integer atomics
 * (histograms, counters, maxima on float bits) are exact and stay.  Scope: one process, one GPU, one binary; slower
 * (docs/design/21-reproducible-training.md has the table).  Off: nothing changes. */
int dvq_set_deterministic(int on);
int dvq_deterministic(void);
/* Process-wide count of launches that took a path whose floating-point result depends on arrival order (float atomics with several
 * writers per address), bumped at the dispatch branch that selects such a kernel or epilogue.  It does not move across a call made in
 * deterministic mode; that it DOES move with the mode off shows a shape really has several writers per address. */
long long dvq_unordered_launches(void);
/* fp32 operands on the bf16 matrix pipe (opt-in; default: environment DVQ_FP32_SPLIT=1, else off): the fp32 instantiations of the
 * convolution / GEMM kernels split every operand element into two bf16 planes (x = hi + lo) in registers and run hi.hi + hi.lo + lo.hi as
 * three v_mfma_f32_32x32x16_bf16 passes with fp32 accumulation instead of v_mfma_f32_32x32x2_f32: ~2^-17 relative error per product
 * (fp32: 2^-24) at 3/16 of the matrix-pipe time.  Activations, statistics, gradients and accumulators stay fp32 (`--dtype fp32x3`). */
int dvq_set_fp32_split(int on);
int dvq_fp32_split(void);
/* Diagnostics for the benchmark's roofline context (allocates, synchronises the stream; NOT for the hot path): TFLOP/s and shader
 * clock (MHz) that a register-only bf16 MFMA loop sustains on every CU for ~3 ms, with all-zero (random_operands = 0) or random
 * bf16 operands -- the power-limited ceiling of the matrix pipes, which depends on the operand bit patterns. */
int dvq_probe_mfma_rate(int random_operands, float* tflops, float* mhz, dvq_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Vector quantisation.  Replaces VQEmbedding.compute_distances + argmin
 * (modules/vector_quantization/quantize2_mask.py:29-55): exact argmin_k |x_n - e_k|^2, lowest k on
 * ties, without materialising the [N,K] distance matrix.
 * ---------------------------------------------------------------------------------------------- */

/* Codebook preparation (once per codebook version): splits e into two bf16 planes, row norms, max
 * norm.  prep must hold dvq_vq_prep_bytes(K,D) bytes. */
size_t dvq_vq_prep_bytes(int64_t K, int64_t D);
int dvq_vq_prepare(const float* codebook, int64_t K, int64_t D, void* prep, dvq_stream_t stream);

/* idx[n] = argmin_k |x[n,:] - codebook[k,:]|^2.  x is [N,D] (row stride D) of `x_dtype`.
 * ws: dvq_vq_argmin_workspace_bytes(N) bytes whose first 256 bytes are ZERO when the call starts: zero a new buffer once; every
 * call leaves them zero again (the re-rank kernel, its last launch, re-arms the counters), so a buffer serves any number of
 * stream-ordered calls without a zero-fill launch.  After the call int32 slots [4], [5], [6] hold the number of rows settled in
 * fp64 over all K codes (generic kernel only), over their candidate list / flagged residue classes, and -- of the latter -- with
 * more candidate classes than an entry lists.  impl: 0 = auto, 1 = force generic VALU kernel, 2 = force MFMA kernel
 * (DVQ_ESHAPE if unsupported) -- this entry's own codes, not the DVQ_IMPL_* of the convolutions and GEMMs. */
size_t dvq_vq_argmin_workspace_bytes(int64_t N);
/* Analysis entry point (VQEmbedding.compute_distances, quantize2_mask.py:29-48): out[n][k] = (|x_n|^2 + |e_k|^2) - 2 x_n.e_k
 * (fp32 FMA arithmetic, the reference's addmm formula), out fp32 [N][K] caller-owned; at most 2^20 rows per call. */
int dvq_vq_distances(const void* x, int x_dtype, const float* codebook, int64_t N, int64_t K, int64_t D, float* out,
                     dvq_stream_t stream);
int dvq_vq_argmin(const void* x, int x_dtype, const float* codebook, const void* prep, int64_t N, int64_t K,
                  int64_t D, int64_t* idx, void* ws, int impl, dvq_stream_t stream);
/* Diagnostic: after the call, the first int32 of `ws` holds the number of rows that took the fp64
 * re-rank path. */

/* x_q[n,:] = x[n,:] + (e[idx[n],:] - x[n,:])  (straight-through forward value, quantize2_mask.py:182)
 * and loss_sum[0] += sum_n mask[n] * |e[idx[n]] - x[n]|^2   (fp64 accumulator; :172-180).
 * mask may be NULL (all ones).  x, x_q: `dtype`; mask fp32 [N]. */
int dvq_vq_gather_loss(const void* x, int dtype, const float* codebook, const int64_t* idx, const float* mask,
                       int64_t N, int64_t D, void* x_q, double* loss_sum, dvq_stream_t stream);
/* VQ backward: dx = g_xq + coef * mask[n] * (x - e[idx[n]]),
 * coef = 2*beta*g_loss/(N*D) read from coef_dev[0] (device scalar). */
int dvq_vq_backward(const void* g_xq, const void* x, int dtype, const float* codebook, const int64_t* idx,
                    const float* mask, const float* coef_dev, int64_t N, int64_t D, void* dx, dvq_stream_t stream);
/* codebook gather: out[n,:] = codebook[idx[n],:]  (VQEmbedding.embed, quantize2_mask.py:130-132) */
int dvq_vq_embed(const float* codebook, const int64_t* idx, int64_t N, int64_t D, int out_dtype, void* out,
                 dvq_stream_t stream);

/* EMA statistics (quantize2_mask.py:66-84): stats[k*(D+1)+d] = sum of x rows assigned to k,
 * stats[k*(D+1)+D] = count.  stats is an fp32 [K,D+1] buffer (zeroed by the call; ONE fused buffer so the
 * data-parallel exchange is ONE all-reduce). */
int dvq_vq_ema_stats(const void* x, int dtype, const int64_t* idx, int64_t N, int64_t K, int64_t D, float* stats,
                     dvq_stream_t stream);
/* EMA apply + dead-code restart + Laplace-smoothed normalisation (quantize2_mask.py:89-115).
 * restart_rows: [K,D] fp32 candidate rows or NULL (restart disabled). weight: [K+1,D] (row K untouched). */
int dvq_vq_ema_apply(const float* stats, const float* restart_rows, float decay, float eps, int64_t K, int64_t D,
                     float* cluster_size_ema, float* embed_ema, float* weight, float* scratch_sum,
                     dvq_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Patch entropy + fixed-entropy gate.  Replaces Entropy.forward
 * (models/stage1_dynamic/dqvae_dual_entropy.py:25-63) and DualGrainFixedEntropyRouter.forward
 * (modules/dynamic_modules/RouterDual.py:53-57).  img: NCHW fp32 [B,3,H,W]; entropy: [B,H/p,W/p] fp32;
 * gate (may be NULL): int64 [B,H/p,W/p,2] = [H<=t, H>t].
 * ---------------------------------------------------------------------------------------------- */
int dvq_patch_entropy_gate(const float* img, int64_t B, int64_t H, int64_t W, int patch, float threshold,
                           float* entropy, int64_t* gate, dvq_stream_t stream);
/* Same with the 32 histogram bins on linspace(bin_lo, bin_hi, 32) instead of the model's (-1, 1): the reference's threshold
 * calibration script bins on (0, 1) (scripts/tools/calculate_entropy_thresholds.py:74) -- scripts/tools of this repo can
 * reproduce either table. */
int dvq_patch_entropy_gate_range(const float* img, int64_t B, int64_t H, int64_t W, int patch, float bin_lo, float bin_hi,
                                 float threshold, float* entropy, int64_t* gate, dvq_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm(32, eps) + swish.  Replaces Normalize + nonlinearity
 * (modules/diffusionmodules/model.py:29-35).  x,y: NHWC [N,HW,C] of `dtype`.
 * stats: fp64 [N,G,2] zeroed by the caller before dvq_gn_stats (sum, sum of squares).
 * ---------------------------------------------------------------------------------------------- */
int dvq_gn_stats(const void* x, int dtype, int64_t N, int64_t HW, int64_t C, int G, double* stats,
                 dvq_stream_t stream);
/* y = act(gn(x)); `silu` is an activation code: 0 none, 1 swish, 2 LeakyReLU(0.2) (see DVQ_ACT_*).  mean_rstd (fp32 [N,G,2]) is written for the backward. */
int dvq_gn_apply(const void* x, int dtype, int64_t N, int64_t HW, int64_t C, int G, float eps, const double* stats,
                 const float* gamma, const float* beta, int silu, void* y, float* mean_rstd, dvq_stream_t stream);
/* backward pass 1: red fp64 [N,G,2] (zeroed) += (sum dz*gamma, sum dz*gamma*xhat); dgamma/dbeta fp32 [C] += .
 * `partials` (may be NULL): caller-owned scratch of dvq_gn_bwd_partial_bytes(N, HW, C) bytes -- every block then stores its
 * sums there and a fold kernel adds them up (no same-address atomic chains); NULL = atomics straight into red / dgamma / dbeta.
 * backward pass 2: dx.  dy: grad w.r.t. y. */
size_t dvq_gn_bwd_partial_bytes(int64_t N, int64_t HW, int64_t C);
int dvq_gn_bwd_reduce(const void* x, const void* dy, int dtype, int64_t N, int64_t HW, int64_t C, int G,
                      const float* mean_rstd, const float* gamma, const float* beta, int silu, double* red,
                      float* dgamma, float* dbeta, float* partials, dvq_stream_t stream);
/* addend (may be NULL): a tensor like dx that is added to the result (gradient of a joining residual branch) */
int dvq_gn_bwd_dx(const void* x, const void* dy, int dtype, int64_t N, int64_t HW, int64_t C, int G,
                  const float* mean_rstd, const float* gamma, const float* beta, int silu, const double* red,
                  const void* addend, void* dx, dvq_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA.  Replaces torch.nn.Conv2d call sites of ResnetBlock /
 * Upsample / Downsample / AttnBlock 1x1 / quant_conv (modules/diffusionmodules/model.py:38-192,
 * models/stage1_dynamic/dqvae_dual_entropy.py:93-94).
 * ---------------------------------------------------------------------------------------------- */
/* Kernel choice of dvq_conv_desc.impl, dvq_gemm_nt and dvq_gemm_tn (dvq_vq_argmin's `impl` keeps its own 0 / 1 / 2 meaning, see there).
 * A REQUIRED code returns DVQ_ESHAPE on a shape its kernel does not run; a PREFERRED code falls through to the automatic choice. */
enum {
    DVQ_IMPL_AUTO = 0,             /* automatic choice */
    DVQ_IMPL_NAIVE = 1,            /* naive_nt_kernel / naive_tn_kernel; runs every shape */
    DVQ_IMPL_MFMA = 2,             /* required. NT: 128 x 128 LDS-DMA igemm_nt_glds; TN: igemm_tn_tr for bf16 operands, igemm_tn for fp32 */
    DVQ_IMPL_REGSTAGE = 3,         /* required. register-staged igemm_nt_kernel / igemm_tn_kernel */
    DVQ_IMPL_HALO = 4,             /* required. conv entries only: the LDS-resident-halo 3 x 3 kernels (conv_halo.hip) */
    DVQ_IMPL_WIDE = 5,             /* preferred. NT: gemm_nt_wide_kernel; TN: as DVQ_IMPL_MFMA */
    DVQ_IMPL_WIDE_PIPE = 6,        /* preferred. NT: 256-row gemm_nt_wide_pipe; TN: gemm_tn_wide_pipe instead of the 8-phase kernel */
    DVQ_IMPL_WIDE_PIPE_4WAVE = 7,  /* preferred. NT: 4-wave gemm_nt_wide_pipe; TN: as DVQ_IMPL_MFMA */
    DVQ_IMPL_WIDE_PIPE_192 = 8,    /* preferred. NT: 192-row gemm_nt_wide_pipe; TN: as DVQ_IMPL_MFMA */
    DVQ_IMPL_CONV_PIPE = 9,        /* required. NT convolutions (bf16): conv_nt_pipe_kernel; TN: as DVQ_IMPL_MFMA */
    DVQ_IMPL_8PHASE = 10           /* preferred. NT: gemm_nt_8phase_kernel; TN: as DVQ_IMPL_MFMA */
};

typedef struct dvq_conv_desc {
    int64_t N;        /* batch */
    int64_t H, W;     /* LOGICAL input height/width (after the optional nearest x2 upsample) */
    int64_t Cin;
    int64_t OH, OW;   /* output height/width */
    int64_t Cout;
    int32_t KH, KW;
    int32_t stride;
    int32_t pad_t, pad_l; /* zero padding top/left; bottom/right padding is implied by OH/OW */
    int32_t upsample; /* 1: the stored input is [N,H/2,W/2,Cin] and is read through nearest x2 (model.py:50);
                       * 2 (dvq_conv2d_fwd / dvq_conv2d_dgrad only, shapes accepted by dvq_conv3x3_subpixel_ok): the same, and the
                       * weight argument carries the sub-pixel pack behind its 3x3 pack (dvq_pack_weight, bit 9 of dtype) */
    int32_t dtype;    /* DVQ_F32 / DVQ_BF16: activations and packed weights */
    int32_t impl;     /* DVQ_IMPL_*: AUTO, NAIVE, MFMA, REGSTAGE, HALO, CONV_PIPE (DVQ_ESHAPE if the shape is not eligible) */
} dvq_conv_desc;

/* Activations fused into conv epilogues / behind a normalisation (dvq_gn_* take the same codes in `silu`):
 * 0 none, 1 swish (GroupNorm only), 2 LeakyReLU(0.2) (PatchGAN, modules/discriminator/model.py:35-62),
 * 3 ReLU (VGG16 of LPIPS, modules/losses/lpips.py:75-93; conv epilogues only). */
enum { DVQ_ACT_NONE = 0, DVQ_ACT_SWISH = 1, DVQ_ACT_LRELU = 2, DVQ_ACT_RELU = 3 };

/* y[n,oh,ow,co] = act(bias[co] + sum x[n,oh*s-pt+kh, ow*s-pl+kw, ci] * w[co,kh,kw,ci] (+ residual)).
 * w: packed [Cout][KH][KW][Cin] of `dtype` (Cin here is the padded count); bias fp32 [Cout] or NULL;
 * residual NHWC like y or NULL.
 * act: DVQ_ACT_NONE / _RELU / _LRELU (nn.Conv2d followed by nn.ReLU / nn.LeakyReLU(0.2)); any other than NONE excludes residual,
 * gn_scale_shift and out_stats (DVQ_EINVAL).
 * Fused GroupNorm on shapes accepted by dvq_conv3x3_fused_ok (bf16, 3x3, stride 1, pad 1, H % 8 == 0, W % 32 == 0,
 * Cin % 64 == 0; DVQ_ESHAPE elsewhere): gn_scale_shift (fp32 [N][Cin][2], from dvq_gn_scale_shift) applies GroupNorm + swish to the
 * INPUT inside the kernel (ResnetBlock's norm -> swish -> conv, model.py:119-129, without materialising the activation);
 * out_stats (fp64 [N][out_groups][2], accumulated) receives sum / sum of squares of the OUTPUT per group, i.e. the
 * statistics pass of the next GroupNorm.  Either may be NULL.
 * scratch, scratch_bytes (here, in dvq_conv2d_dgrad and in dvq_conv2d_wgrad; NULL, 0 is always legal): see dvq_conv2d_scratch_bytes. */
int dvq_conv3x3_fused_ok(const dvq_conv_desc* d);
/* Nearest x2 upsample + 3x3 as four 2x2 sub-pixel convolutions.  The upsampled image holds every source pixel four times, so an output
 * pixel of parity class (py, px) reads 2 x 2 distinct source pixels: out[2i+py][2j+px] = sum_{a,b in {0,1}} Weff[py][px][a][b] .
 * x[i+a+py-1][j+b+px-1], with Weff the sums of the 3x3 taps that land on the same source pixel (rows: py = 0: a = 0 <- {0}, a = 1 <-
 * {1, 2}; py = 1: a = 0 <- {0, 1}, a = 1 <- {2}; columns alike), summed in fp32 and rounded once: 4/9 of the multiply-adds, and an
 * input gradient that is formed at the low resolution (no workspace, no 2x2 sum pass).  Results are within bf16 rounding of the 9-tap
 * form, not bit-identical to it.  dvq_conv3x3_subpixel_ok: 1 for descriptors with upsample != 0 that dvq_conv2d_fwd (without residual,
 * gn_scale_shift or activation; with them it runs the 9-tap form on the 3x3 pack) and dvq_conv2d_dgrad run this way when upsample == 2:
 * bf16, 3x3 / stride 1 / pad 1, (H/2) % 8 == 0, (W/2) % 32 == 0, Cin % 64 == 0, Cout % 64 == 0, impl AUTO or HALO.  The weight
 * gradient, fp32 and fp32x3 keep upsample == 1. */
int dvq_conv3x3_subpixel_ok(const dvq_conv_desc* d);
int dvq_conv2d_fwd(const dvq_conv_desc* d, const void* x, const void* w, const float* bias, const void* residual, void* y,
                   const float* gn_scale_shift, double* out_stats, int out_groups, int act, void* scratch, int64_t scratch_bytes,
                   dvq_stream_t stream);
/* fp32x3 at LAUNCH level (dvq_set_fp32_split on, descriptor dtype DVQ_F32, impl DVQ_IMPL_AUTO): the three passes below take `scratch`
 * and run the split scheme's three products on the bf16 kernels, from bf16 planes hi = RNE(v), lo = RNE(v - hi) written into it.
 *   DVQ_PASS_FWD / DVQ_PASS_DGRAD: 3 x 3, stride 1, pad 1 with H % 8 == 0, W % 32 == 0, streamed channels % 64 == 0 and produced channels
 *     a multiple of 4 (>= 4).  The planes lie side by side on the channel axis ([x_hi | x_lo | x_hi] against [w_hi | w_hi | w_lo]); ONE
 *     launch of the bf16 halo kernel with fp32 residual / gate / activation and fp32 output.  Not with gn_scale_shift or out_stats.
 *   DVQ_PASS_WGRAD: any geometry the bf16 weight gradient takes (channels re-padded from 4 to 8).  x_lo.dy_hi + x_hi.dy_lo + x_hi.dy_hi
 *     as ONE halo launch over the planes, or three launches of the bf16 weight-gradient path.  Not with gn_scale_shift.
 * dvq_conv2d_scratch_bytes: the bytes that route wants under the CURRENT dvq_fp32_split() state; 0 when no route wants scratch (bf16
 * operands, the split off, impl != DVQ_IMPL_AUTO, a FWD / DGRAD shape outside the list above).  Routing, where the query is not 0:
 *   scratch != NULL: the launch-level scheme.  scratch_bytes below the query or a pointer that is not 16-B aligned: DVQ_EWORKSPACE from
 *     the argument check, before any launch.
 *   scratch == NULL: the route that needs none (the fp32 kernel that splits at every fragment read).  A legal choice, not an error.
 * Where the query is 0 both arguments are ignored.
 * dvq_split_bf16_planes: x fp32 [rows][cin] -> two bf16 [rows][cout] tensors (cin % 4 == 0, cout % 8 == 0, cout >= cin; channels >= cin
 * are zero). */
enum { DVQ_PASS_FWD = 0, DVQ_PASS_DGRAD = 1, DVQ_PASS_WGRAD = 2 };
int64_t dvq_conv2d_scratch_bytes(const dvq_conv_desc* d, int pass);
int dvq_split_bf16_planes(const float* x, void* hi, void* lo, int64_t rows, int64_t cin, int64_t cout, dvq_stream_t stream);
/* scale_shift[n][c] = {rstd*gamma, beta - mean*rstd*gamma} from the fp64 statistics; mean_rstd (fp32 [N][G][2]) optional */
int dvq_gn_scale_shift(const double* stats, const float* gamma, const float* beta, int64_t N, int64_t HW, int64_t C, int G,
                       float eps, float* scale_shift, float* mean_rstd, dvq_stream_t stream);

/* dx (stored-input shape, i.e. [N,H/2,W/2,Cin] when upsample) from dy [N,OH,OW,Cout].
 * wt: weights in IHWO layout [d->Cin,KH,KW,Cout] of `dtype` (dvq_pack_weight writes the first Cin_real rows; when the
 * descriptor's Cin is channel-padded the caller provides zero rows up to d->Cin).  When upsample is 1,
 * ws must hold N*H*W*Cin elements of `dtype` (gradient at the upsampled resolution); with upsample == 2 ws is not used (may be NULL).
 * mask (may be NULL): dgrad through the conv AND the activation that produced the conv's input: mask = that activation's OUTPUT
 * (same shape as dx); dx = dgrad * (mask > 0 ? 1 : slope(mask_act)), mask_act DVQ_ACT_RELU / _LRELU, no folded upsample. */
int dvq_conv2d_dgrad(const dvq_conv_desc* d, const void* dy, const void* wt, void* dx, void* ws, const void* mask, int mask_act,
                     void* scratch, int64_t scratch_bytes, dvq_stream_t stream);

/* Weight gradient, ACCUMULATED straight into the fp32 gradient of the reference-layout parameter (zero it first; no packed
 * intermediate, no unpack pass); d->Cin / d->Cout are the padded channel counts of x / dy, cin_real / cout_real those of the parameter.
 * ohwi = 0: grad is [cout][cin][KH][KW] (torch-contiguous parameter); ohwi = 1: grad is stored [cout][KH][KW][cin]
 * (the trainer's flat storage keeps conv weights and their gradients channel-last: contiguous atomics, no unpack).
 * dvq_pack_weight(_s_multi) accept the same storage with bit 8 of `dtype` set.
 * dbias: fp32 [cout_real], accumulated, may be NULL.  gn_scale_shift (may be NULL; shapes accepted by dvq_conv3x3_fused_ok): the
 * GroupNorm + swish the forward fused into its prologue, re-applied to x inside the kernel. */
int dvq_conv2d_wgrad(const dvq_conv_desc* d, const void* x, const void* dy, int64_t cin_real, int64_t cout_real, float* grad,
                     float* dbias, int ohwi, const float* gn_scale_shift, void* scratch, int64_t scratch_bytes, dvq_stream_t stream);

/* Pack every conv weight of a model in ONE launch.  table_dev: device array of n_entries records
 * { const float* master; void* w; void* wt; int64 Cout, Cin, taps, Cin_p, Cout_p, begin, dtype } where `begin` is
 * the exclusive prefix sum of (Cout*taps*Cin_p [if w] + Cin*taps*Cout_p [if wt]) and total_work the full sum.
 * Cin_p and Cout_p must be multiples of 4 (the kernel moves four destination elements per thread); DVQ_EINVAL otherwise is NOT
 * checked on the device table: the caller pads channels to the vector width of the dtype (4 fp32 / 8 bf16) anyway. */
int dvq_pack_weights_multi(const void* table_dev, int64_t n_entries, int64_t total_work, dvq_stream_t stream);
/* The same for nn.Linear weights (stackgpt.py:44-96): table_dev = device array of n_entries records
 * { const float* master [out][in]; bf16* w [out_p][in]; bf16* wt [in][out_p]; int64 out, in, out_p, tile_begin, wt_ld;
 *   const float* bias_src; float* bias_dst } with out_p a multiple of
 * 8 (rows >= out of w and columns >= out of wt are written as zero), tile_begin the exclusive prefix sum of
 * ceil(out_p / 64) * ceil(in / 64) and total_tiles the full sum: ONE launch per optimizer step instead of a cast + a transpose per layer.
 * wt_ld: row pitch of wt (0 = out_p); bias_src / bias_dst (may be null): the layer's fp32 bias copied into a slice of a concatenated
 * bias -- both serve projections that share their input and run as ONE GEMM over row-concatenated weights (key / query / value). */
int dvq_linear_pack_multi(const void* table_dev, int64_t n_entries, int64_t total_tiles, dvq_stream_t stream);

/* weight packing: master fp32 OIHW (the reference's nn.Conv2d parameter layout) -> `dtype`
 * w [Cout][KH][KW][Cin_p] (forward / wgrad layout) and wt [Cin][KH][KW][Cout_p] (dgrad layout), zero padded
 * to Cin_p / Cout_p channels (multiples of 8 for bf16, 4 for fp32); either output may be NULL.
 * Bit 9 of dtype (3x3 kernels, Cin_p == Cin, Cout_p == Cout, both outputs given; the table entries of dvq_pack_weights_multi alike,
 * whose `begin` then counts 16*Cout*Cin more elements per output): the sub-pixel packs of dvq_conv3x3_subpixel_ok are written BEHIND
 * the 3x3 packs -- Weff [class 2py+px][Cout][tap 2a+b][Cin] at w + Cout*9*Cin and WeffT [Cin][class][tap][Cout] at wt + Cin*9*Cout,
 * each element the fp32 sum of its group's taps (rows then columns, ascending) rounded once. */
int dvq_pack_weight(const float* master, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW, int64_t Cin_p,
                    int64_t Cout_p, int dtype, void* w, void* wt, dvq_stream_t stream);
/* grad_oihw[co][ci][kh][kw] += dw[co][kh][kw][ci]   (dw: the fp32 [Cout][KH][KW][Cin_p] output of wgrad) */
int dvq_unpack_wgrad(const float* dw, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW, int64_t Cin_p, float* grad,
                     dvq_stream_t stream);
/* image layout: NCHW fp32 [B,C,H,W] <-> NHWC `dtype` [B,H,W,Cp] (channels zero-padded to Cp) */
int dvq_nchw_to_nhwc_pad(const float* in, int64_t B, int64_t C, int64_t H, int64_t W, int64_t Cp, int dtype, void* out,
                         dvq_stream_t stream);
int dvq_nhwc_pad_to_nchw(const void* in, int dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t Cp, float* out,
                         dvq_stream_t stream);

/* Generic batched GEMM on the same kernels.
 * NT:  C[b][m][n] = alpha * sum_k A[b][m][k] * B[b][n][k] (+ bias) ; bias_mode 0 none, 1 per-n, 2 per-m.
 * TN:  C[b][i][j] (fp32, accumulated) += sum_m A[b][m][i] * B[b][m][j].
 * Strides in elements.  impl: DVQ_IMPL_*. */
int dvq_gemm_nt(const void* A, const void* B, void* C, int dtype, int64_t M, int64_t N, int64_t K, int64_t lda,
                int64_t ldb, int64_t ldc, int64_t batch, int64_t sA, int64_t sB, int64_t sC, float alpha,
                const float* bias, int bias_mode, int impl, dvq_stream_t stream);
/* colsum (may be NULL; batch 1 only): colsum[i] += sum_m A[m][i] from the same pass over A (bias gradient of a Linear layer next to
 * its weight gradient: torch.nn.Linear's autograd, stackgpt.py:44-96) */
int dvq_gemm_tn(const void* A, const void* B, float* C, float* colsum, int dtype, int64_t Mred, int64_t I, int64_t J, int64_t lda,
                int64_t ldb, int64_t ldc, int64_t batch, int64_t sA, int64_t sB, int64_t sC, int impl, dvq_stream_t stream);

/* Register a caller-owned device scratch buffer (one per process; the library cuts it into eight slots, one per stream that
 * uses it, so the side-stream weight gradients and the main stream never share one).  With >= 76 MiB per slot the split-K
 * weight-gradient kernels store per-workgroup partial tiles with plain writes and fold them in a second kernel instead of
 * issuing cross-XCD fp32 atomics.  ptr = NULL, bytes = 0 unregisters.
 * Slot ownership: a stream keeps its slot; a slot handed out while the stream was CAPTURING is pinned (the recorded graph holds
 * its address) until dvq_workspace_release(stream); an unpinned slot is re-assigned to a new stream only when its owner is idle,
 * least recently used first; a stream that finds no slot gets none (atomics). */
int dvq_set_workspace(void* ptr, int64_t bytes);
int dvq_workspace_release(dvq_stream_t stream);

/* ---- launch lists: a recorded step re-issued as plain stream launches -----------------------------------------------
 * The training step of the reference is driven by pytorch-lightning, one Python call per operator per step (train.py:233-262,
 * models/stage1_dynamic/dqvae_dual_entropy.py:123-150); here the step's launch sequence is static, is recorded once by HIP stream
 * capture, and is replayed from C.  dvq_cmdlist_create walks a captured hipGraph_t (kernel / memset / memcpy / empty nodes) into
 * a flat operation array: nodes keep their capture order, the fork / join structure of a two-stream capture is mapped onto two
 * streams with event pairs at the cross-stream edges.  dvq_cmdlist_replay issues the array with hipLaunchKernel on (main, side):
 * the device sees what an eagerly launched step puts in its queues (hipGraphLaunch adds ~7 % on a 2400-kernel step on ROCm 7.2).
 * The list borrows the argument blocks held by the graph's nodes: destroy the list before the graph.
 * dvq_cmdlist_info: {kernel launches, of those on the side stream, event waits, memset + memcpy operations | side_open << 32}. */
int dvq_cmdlist_create(void* hip_graph, dvq_cmdlist_t* out);
int dvq_cmdlist_replay(dvq_cmdlist_t list, dvq_stream_t main_stream, dvq_stream_t side_stream);
int dvq_cmdlist_info(dvq_cmdlist_t list, int64_t* info4);
int dvq_cmdlist_destroy(dvq_cmdlist_t list);

/* ---- loss networks (LPIPS + PatchGAN), modules/losses/lpips.py, modules/discriminator/model.py -------------------
 * BatchNorm2d (training mode) = dvq_gn_* with N=1, HW=N*H*W, G=C (one group per channel over the whole batch). */
/* ScalingLayer (lpips.py:53-61) and its backward: y[..,c] = x[..,c]*a[c] + b[c]  (b may be NULL); n = total elements */
int dvq_affine_channels(const void* x, int dtype, int64_t n, int64_t C, const float* a, const float* b, void* y,
                        dvq_stream_t stream);
/* y = a + scale_dev[0] * b  (generator-loss weighting with the device-resident adaptive weight,
 * vqperceptual_multidisc.py:97-107,139); n % 8 == 0 */
int dvq_axpy_dev(const void* a, const void* b, const float* scale_dev, int dtype, int64_t n, void* y, dvq_stream_t stream);
/* nn.MaxPool2d(2,2) of VGG16 on NHWC: x [N,2h,2w,C] -> y [N,h,w,C] */
int dvq_maxpool2x2(const void* x, int dtype, int64_t N, int64_t h, int64_t w, int64_t C, void* y, dvq_stream_t stream);
/* backward of ReLU -> {feature tap, max-pool}: dz = (route(dpool) + dtap) * (a > 0); a = ReLU output [N,2h,2w,C],
 * dpool [N,h,w,C] or NULL, dtap like a or NULL; ties go to the first maximum in scan order (torch semantics) */
int dvq_maxpool2x2_relu_bwd(const void* a, const void* dpool, const void* dtap, int dtype, int64_t N, int64_t h, int64_t w,
                            int64_t C, void* dz, dvq_stream_t stream);
/* LPIPS head of one tap (lpips.py:41-50,113-121): val[n] += mean_p sum_c lin[c]*(f0/(|f0|+1e-10) - f1/(|f1|+1e-10))^2;
 * df1 (NULL to skip) = gscale * d val[n] / d f1, gated by f1 > 0.  C in {64,128,256,512}. */
int dvq_lpips_head(const void* f0, const void* f1, const float* lin, int dtype, int64_t N, int64_t HW, int64_t C, float* val,
                   float gscale, void* df1, dvq_stream_t stream);
/* the same with NetLinLayer's nn.Dropout(p_drop) on the squared differences (lpips.py:64-70; the reference leaves it active while
 * training): element (n, pixel, channel) kept iff dvq_hash32 of (seed, element index) >= p_drop * 2^32, kept terms scaled by
 * 1 / (1 - p_drop), in the value and in df1 alike.  p_drop == 0: identical to dvq_lpips_head. */
int dvq_lpips_head_drop(const void* f0, const void* f1, const float* lin, int dtype, int64_t N, int64_t HW, int64_t C, float* val,
                        float gscale, void* df1, float p_drop, uint64_t seed, dvq_stream_t stream);

/* ---- feature-routed (Gumbel) dual / triple grain pieces: RouterDual.py:6-43, RouterTriple.py:6-56,
 * EncoderDual.py:130-156, EncoderTriple.py:143-183 ------------------------------------------------------------------ */
/* nn.AvgPool2d(k) (k in 1,2,4) of x [N,h*k,w*k,C] written into the channel slice [coff, coff+C) of rows of ldy channels
 * (= torch.cat(..., dim=1).permute(0,2,3,1) of the router input without materialising the pieces); and its backward */
int dvq_avgpool_slice(const void* x, int dtype, int64_t N, int64_t h, int64_t w, int64_t C, int k, void* y, int64_t ldy,
                      int64_t coff, dvq_stream_t stream);
int dvq_avgpool_slice_bwd(const void* dy, int dtype, int64_t ldy, int64_t coff, int64_t N, int64_t h, int64_t w, int64_t C,
                          int k, void* dx, dvq_stream_t stream);
/* nn.SiLU of the router MLP and its backward (x = pre-activation); n % 8 == 0 */
int dvq_silu(const void* x, int dtype, int64_t n, void* y, dvq_stream_t stream);
int dvq_silu_bwd(const void* x, const void* dy, int dtype, int64_t n, void* dx, dvq_stream_t stream);
/* nn.ReLU of the gate_type="2layer-fc-ReLu" router MLP (RouterTriple.py:23-28) and its backward (x = pre-activation); n % 8 == 0 */
int dvq_relu(const void* x, int dtype, int64_t n, void* y, dvq_stream_t stream);
int dvq_relu_bwd(const void* x, const void* dy, int dtype, int64_t n, void* dx, dvq_stream_t stream);
/* Upsample(with_conv=False) (modules/diffusionmodules/model.py:49-53): F.interpolate(scale_factor=2, mode="nearest"), NHWC
 * x [N,h,w,C] -> y [N,2h,2w,C]; backward dx[n,i,j] = sum of dy over the 2 x 2 footprint.  C % 8 == 0.
 * (Downsample(with_conv=False) = avg_pool2d(2, 2), model.py:73-74, is dvq_avgpool_slice / _bwd with k = 2.) */
int dvq_upsample_nearest2x(const void* x, int dtype, int64_t N, int64_t h, int64_t w, int64_t C, void* y, dvq_stream_t stream);
int dvq_upsample_nearest2x_bwd(const void* dy, int dtype, int64_t N, int64_t h, int64_t w, int64_t C, void* dx, dvq_stream_t stream);
/* S-grain merge (S = 2, 3).  heads[l]: [N, hc<<l, wc<<l, C] (l = 0 coarsest); idx int64 [N,hc,wc] = selected level of each
 * coarsest cell; out [N, hc<<(S-1), wc<<(S-1), C] = nearest-upsampled selected head (* scale[cell] if scale != NULL, the
 * straight-through gate_grad); mask (optional) fp32 [N,hf,wf] = 4^-(S-1-level) (codebook mask).
 * Backward: dheads[l] = scale * (sum of g over each pixel's footprint where selected, else 0); dscale[cell] (optional) =
 * sum g * selected head value. */
int dvq_grain_merge(const void* const* heads, int S, const int64_t* idx, const float* scale, int dtype, int64_t N, int64_t hc,
                    int64_t wc, int64_t C, void* out, float* mask, dvq_stream_t stream);
int dvq_grain_merge_bwd(const void* g_out, const void* const* heads, int S, const int64_t* idx, const float* scale, int dtype,
                        int64_t N, int64_t hc, int64_t wc, int64_t C, void* const* dheads, float* dscale, dvq_stream_t stream);

/* ---- stage-2 input permutation (integer, bit-exact): DualGrainSeperatePermuter, modules/dynamic_modules/permuter.py:50-135 -----
 * forward: indices int64 [B, hw1*hw2, hw1*hw2] (codes), grain int64 [B,hw1,hw1] (0 coarse / 1 fine) -> EOS-terminated,
 * PAD-filled rows of the MAXIMUM length: coarse_content / coarse_position [B, hw1^2 + 1], fine_content / fine_position
 * [B, (hw1*hw2)^2 + 1]; counts int32 [B][2] = number of coarse cells / fine codes of each image (the caller narrows the
 * rows to max(count)+1 like pad_sequence does).  order 0 = "region-first", 1 = "row-first" (hw2 must be 2). */
int dvq_permute_dual(const int64_t* indices, const int64_t* grain, int64_t B, int hw1, int hw2, int order, int64_t content_pad,
                     int64_t content_eos, int64_t cpos_pad, int64_t cpos_eos, int64_t fpos_pad, int64_t fpos_eos,
                     int64_t* coarse_content, int64_t* coarse_position, int64_t* fine_content, int64_t* fine_position,
                     int* counts, dvq_stream_t stream);
/* forward_back: sequences [B,Lc] / [B,Lf] -> code map int64 [B, hw1*hw2, hw1*hw2].  Coarse codes are broadcast to their
 * cells only when the coarse EOS is present, entries at and after the first EOS are ignored, a position written twice
 * keeps the last write (the reference's sequential semantics). */
int dvq_permute_dual_back(const int64_t* coarse_content, const int64_t* fine_content, const int64_t* coarse_position,
                          const int64_t* fine_position, int64_t B, int64_t Lc, int64_t Lf, int hw1, int hw2, int64_t cpos_eos,
                          int64_t fpos_eos, int64_t* out, dvq_stream_t stream);

/* row softmax (AttnBlock, model.py:182) and its backward, rows of length L, in place allowed */
int dvq_softmax_rows(const void* s, int dtype, int64_t rows, int64_t L, float scale, void* p, dvq_stream_t stream);
int dvq_softmax_rows_bwd(const void* p, const void* dp, int dtype, int64_t rows, int64_t L, float scale, void* ds,
                         dvq_stream_t stream);
/* batched 2-D transpose: out[b][c][r] = in[b][r][c] */
int dvq_transpose(const void* in, int dtype, int64_t batch, int64_t R, int64_t C, void* out, dvq_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Element-wise / small ops of the path
 * ---------------------------------------------------------------------------------------------- */
/* Dual-grain merge (EncoderDual.py:134-149): h_dual = grain? h_fine : up2(h_coarse); mask = grain?1:.25.
 * h_fine [B,2h,2w,C], h_coarse [B,h,w,C], grain int64 [B,h,w] (1 = fine). mask fp32 [B,2h,2w]. */
int dvq_dual_merge(const void* h_fine, const void* h_coarse, const int64_t* grain, int dtype, int64_t B, int64_t h,
                   int64_t w, int64_t C, void* h_dual, float* mask, dvq_stream_t stream);
int dvq_dual_merge_bwd(const void* g_dual, const int64_t* grain, int dtype, int64_t B, int64_t h, int64_t w,
                       int64_t C, void* g_fine, void* g_coarse, dvq_stream_t stream);
/* y = a + b (same dtype), y = x + bias[hw,c] broadcast over batch (decoder position bias) */
int dvq_add(const void* a, const void* b, int dtype, int64_t n, void* y, dvq_stream_t stream);
int dvq_add_bias_bcast(const void* x, const float* bias, int dtype, int64_t batch, int64_t inner, void* y,
                       dvq_stream_t stream);
/* 8-channel bf16 pixels: y[p][c] = a[p][c] + (c >= shift ? b[p][c - shift] : 0) -- two 3-channel image gradients side by side in one
 * padded tensor (calculate_adaptive_weight, vqperceptual_multidisc.py:97-107: both last-layer gradients from ONE weight-gradient call) */
int dvq_channel_shift_add8(const void* a, const void* b, int dtype, int64_t npix, int shift, void* y, dvq_stream_t stream);
/* sum over batch: out[inner] (fp32, accumulated) += sum_b x[b][inner] */
int dvq_sum_batch(const void* x, int dtype, int64_t batch, int64_t inner, float* out, dvq_stream_t stream);
/* 2x2 sum pool NHWC (backward of nearest x2): out[n,h,w,c] = sum in[n,2h+a,2w+b,c] */
int dvq_sumpool2x2(const void* in, int dtype, int64_t N, int64_t h, int64_t w, int64_t C, void* out,
                   dvq_stream_t stream);
/* dtype casts */
int dvq_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, dvq_stream_t stream);
/* L1 reconstruction loss (vqperceptual_multidisc.py:116): loss_sum(fp64) += sum |x - xrec|,
 * g[i] = scale_dev[0] * sign(xrec - x) when g != NULL.  x,xrec fp32 NCHW. */
int dvq_l1_loss(const float* x, const float* xrec, int64_t n, double* loss_sum, const float* scale_dev, float* g,
                dvq_stream_t stream);
/* fused Adam over one flat fp32 tensor (torch.optim.Adam semantics, no weight decay / amsgrad) */
int dvq_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
             int step, dvq_stream_t stream);
/* torch.optim.AdamW (decoupled weight decay: p *= 1 - lr*wd before the Adam update), models/stage2_dynamic/
 * dqtransformer_uncond_entropy.py:92-128 */
int dvq_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
              float weight_decay, int step, dvq_stream_t stream);

/* ---- StackGPT building blocks (modules/dynamic_modules/stackgpt.py) ------------------------------------------------- */
/* nn.LayerNorm(C) over rows [rows, C]; mean_rstd fp32 [rows][2] (optional) is what the backward needs */
int dvq_layernorm_fwd(const void* x, int dtype, int64_t rows, int64_t C, float eps, const float* gamma, const float* beta, void* y,
                      float* mean_rstd, dvq_stream_t stream);
/* dx written; dgamma / dbeta (fp32 [C]) accumulated into */
int dvq_layernorm_bwd(const void* x, const void* dy, int dtype, int64_t rows, int64_t C, const float* mean_rstd, const float* gamma,
                      void* dx, float* dgamma, float* dbeta, dvq_stream_t stream);
/* the same with the gradient that by-passes the normalisation added in: dx = layernorm_bwd(..) + dres (dres may be NULL) -- the
 * residual stream of a transformer block (stackgpt.py:80-96) without a separate add pass */
int dvq_layernorm_bwd_res(const void* x, const void* dy, const void* dres, int dtype, int64_t rows, int64_t C, const float* mean_rstd,
                          const float* gamma, void* dx, float* dgamma, float* dbeta, dvq_stream_t stream);
/* the same with a SECOND output dx_drop = dropout(dx, p_drop, seed) (the decisions of dvq_dropout on the same tensor: element index =
 * row * C + column): the backward of the nn.Dropout that sits between this gradient and its next consumer (stackgpt.py:66-69,91-96)
 * without its own pass.  dx_drop NULL: identical to dvq_layernorm_bwd_res. */
int dvq_layernorm_bwd_res_drop(const void* x, const void* dy, const void* dres, int dtype, int64_t rows, int64_t C, const float* mean_rstd,
                               const float* gamma, void* dx, float* dgamma, float* dbeta, void* dx_drop, float p_drop, uint64_t seed,
                               dvq_stream_t stream);
/* nn.GELU() (exact erf form) and its backward (x = pre-activation) */
int dvq_gelu(const void* x, int dtype, int64_t n, void* y, dvq_stream_t stream);
int dvq_gelu_bwd(const void* x, const void* dy, int dtype, int64_t n, void* dx, dvq_stream_t stream);
/* softmax(scale * s) over rows of length L with the causal mask of CausalSelfAttention (stackgpt.py:59-63): row r of a
 * [Tq x L] score matrix (r = row %% Tq) sees columns <= r + offset; masked probabilities are written as 0.
 * Backward: dvq_softmax_rows_bwd on the result. */
int dvq_softmax_causal(const void* s, int dtype, int64_t rows, int64_t L, int64_t Tq, int64_t offset, float scale, void* p,
                       dvq_stream_t stream);
/* nn.Embedding forward: out[b][t0+j][:] (+)= table[idx[b*idx_bstride + j]][:], j < len; out is [B][Ttot][C] of `dtype`,
 * table fp32 [V][C].  Backward: dtable[idx] += dout rows, skipping idx == padding_idx (fp32 atomics; V = table rows selects
 * the per-table-row kernel, V == 0 the per-token one). */
int dvq_embed_gather(const int64_t* idx, int64_t idx_bstride, const float* table, int dtype, int64_t B, int64_t len, int64_t Ttot,
                     int64_t t0, int64_t C, int accumulate, void* out, dvq_stream_t stream);
int dvq_embed_scatter_add(const int64_t* idx, int64_t idx_bstride, const void* dout, int dtype, int64_t B, int64_t len, int64_t Ttot,
                          int64_t t0, int64_t C, int64_t padding_idx, int64_t V, float* dtable, dvq_stream_t stream);
/* F.cross_entropy(logits[:, :V], target, ignore_index) pieces: loss_sum / count (fp32 device scalars, accumulated) and,
 * when dlogits != NULL, dlogits = (softmax - onehot) * gscale_dev[0] (0 on ignored rows and on columns >= V; row stride ldl) */
int dvq_cross_entropy(const void* logits, int dtype, int64_t rows, int64_t V, int64_t ldl, const int64_t* target, int64_t ignore_index,
                      float* loss_sum, float* count, const float* gscale_dev, void* dlogits, dvq_stream_t stream);
/* The token rule: which columns of a logits row [V] the sampler may draw and the token codec gives a frequency to.  ONE definition
 * for both (csrc/token_rule.h): the codec decodes only what it coded under the rule the sampler draws under.
 *   A LIVE row (finished == NULL or finished[row] == 0) masks column c when c is listed in forbid_idx[row][0 .. n_forbid) (entries
 *   outside [0, V) are ignored), or c >= forbid_from, or c is one of forbid_codes4[0 .. 3]; then keep_code gets its logit back; then
 *   late_forbid_code is masked -- in this order, so late_forbid_code wins over keep_code.
 *   A FINISHED row (finished[row] != 0) keeps pad_code only.
 * -1 is an unused code (forbid_codes4[i], keep_code, late_forbid_code); forbid_from < 0 or > V means V: no bound.  pad_code lies in
 * [0, V).  forbid_idx (int64 [rows][forbid_ld], row pitch forbid_ld >= n_forbid; NULL: no list) and finished (fp32 [rows]; NULL: every
 * row is live) are DEVICE pointers; everything else is read on the host during the call and copied by value into the kernel arguments,
 * so a call recorded by stream capture does not depend on the struct afterwards.  B and n_forbid stay below 2^30. */
#define DVQ_TOKEN_RULE_MAXV 2048 /* the most columns (V) the entry points that take a dvq_token_rule accept */
typedef struct dvq_token_rule {
    const int64_t* forbid_idx;
    int64_t n_forbid, forbid_ld, forbid_from, forbid_codes4[4], keep_code, late_forbid_code, pad_code;
    const float* finished;
} dvq_token_rule;
/* Fused constrained sampling of one token per row (Dualformer's sampler tail: dqtransformer_uncond_entropy.py:522-561 mask rules,
 * models/stage2/utils.py:22-40 top-k / top-p, :328,350 softmax + multinomial / top-1) in ONE launch.  logits [B][ldl] (V <=
 * DVQ_TOKEN_RULE_MAXV columns used), divided by `temperature`, masked by `rule` (dvq_token_rule above).  top_k == 0 / top_p outside
 * (0, 1): filter off.  sample != 0: a draw from the filtered distribution with the device-resident generator `state` (uint64 [2]: key,
 * counter; the counter is advanced by the call -- capturable in a hipGraph); sample == 0: the most probable column (lowest index on
 * ties).  out int64 [B]. */
int dvq_sample_constrained(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, float temperature, const dvq_token_rule* rule,
                           int top_k, float top_p, int sample, uint64_t* state, int64_t* out, dvq_stream_t stream);
/* Classifier-free-guided form of dvq_sample_constrained: B is the number of PAIRS.  logits rows [0, B) are the conditional logits c,
 * rows [B, 2B) the unconditional (null-class) logits u (row pitch ldl).  Per pair and column, in fp32,
 * g = fmaf(1 - guidance, u, guidance * c) (guidance = 1: exactly c; 0: exactly u); then dvq_sample_constrained's pipeline on g
 * (x 1/temperature, the rule, top-k, softmax, top-p, draw).  rule->forbid_idx / rule->finished are read for rows [0, B) only (pass the
 * 2B-row arrays); the uniform of pair i is that of row i; the counter advances once per call.  The token is written to out[i] AND
 * out[i + B] (out int64 [2B]): both halves of the batch carry the same history.  guidance must be finite. */
int dvq_sample_guided(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, float guidance, float temperature,
                      const dvq_token_rule* rule, int top_k, float top_p, int sample, uint64_t* state, int64_t* out, dvq_stream_t stream);
/* Fused causal multi-head self-attention (bf16, head_dim 64 or 128) -- CausalSelfAttention.forward, stackgpt.py:41-69:
 *   out = attn_drop(softmax(causal_mask(q k^T * scale))) v      per (batch, head), scores never materialised.
 * q, k, v, dq, dk, dv: [B*T] rows of n_head*head_dim columns (head h = columns h*head_dim ..), ldqkv elements between consecutive rows.
 * ldqkv == n_head*head_dim: contiguous.  Head size 128 also takes a larger pitch (a multiple of 8, T * ldqkv * 2 < 2^32), e.g.
 * 3 * n_head * head_dim when the three are column blocks of one fused [B*T][3 C] projection output (stackgpt.py:46-48 computes them as
 * three Linear layers over the same input: one GEMM here) and the three gradients are written as column blocks of one [B*T][3 C]
 * matrix that feeds ONE input-gradient GEMM.  out, dout: [B*T][n_head*head_dim], always contiguous.  T % 8 == 0.
 * lse: fp32 [B][n_head][T] (forward output, backward input); p_drop / seed: attention dropout (element index of the
 * [B][n_head][T][T] probability tensor, same generator as dvq_dropout; p_drop == 0: none).
 * scratch: dvq_attn_causal_scratch_bytes(B, T, n_head, head_dim, backward) bytes of device memory -- what the kernels that run need:
 * head size 64 its channel-major operand copies (one forward, three backward) and rowsum(dO * O) behind them; head sizes 128 and 256
 * nothing forward and rowsum(dO * O) alone backward (B * n_head * T floats, rounded up to 256 bytes).  NULL exactly when that is 0.
 * drop_mask (may be NULL): dvq_attn_causal_mask_bytes(B, T, n_head) bytes; the forward stores its keep decisions there, one bit per
 * (query, key) of every causal 32 x 32 tile, and a backward given the same buffer reads them instead of hashing every element again
 * in each of its three kernels (identical results: test_fused_attention_drop_mask_equals_rehash).  NULL: decisions recomputed.
 * DVQ_ESHAPE when dtype / head_dim are not bf16 / 64 or 128 (callers use the per-head GEMM path then) or the pitch is not taken.
 * dvq_attn_causal_ok: 1 when the entry points below take this geometry with contiguous rows (the check they make themselves), else 0. */
int dvq_attn_causal_ok(int dtype, int64_t B, int64_t T, int n_head, int head_dim);
int64_t dvq_attn_causal_scratch_bytes(int64_t B, int64_t T, int n_head, int head_dim, int backward);
int64_t dvq_attn_causal_mask_bytes(int64_t B, int64_t T, int n_head);
int dvq_attn_causal_fwd(const void* q, const void* k, const void* v, int64_t ldqkv, int dtype, int64_t B, int64_t T, int n_head,
                        int head_dim, float scale, float p_drop, uint64_t seed, void* out, float* lse, void* scratch, void* drop_mask,
                        dvq_stream_t stream);
int dvq_attn_causal_bwd(const void* q, const void* k, const void* v, int64_t ldqkv, const void* out, const void* dout, const float* lse,
                        int dtype, int64_t B, int64_t T, int n_head, int head_dim, float scale, float p_drop, uint64_t seed, void* dq,
                        void* dk, void* dv, void* scratch, const void* drop_mask, dvq_stream_t stream);
/* Single-head FULL (non-causal) self-attention of the DQ-VAE's AttnBlock (modules/diffusionmodules/model.py:168-192:
 * w = softmax_j(q^T k * C^-1/2), h = v w^T) for C = 256 (bf16, T %% 32 == 0): the same flash kernels as causal head size 128 with one
 * head of size C, no mask, no dropout; q, k, v, out [B*T][C]; lse fp32 [B][T].  The [B,T,T] score tensor never reaches HBM.  Other
 * shapes (C = 512) return DVQ_ESHAPE: the caller keeps the GEMM + softmax path for them -- dvq_attn_full_ok tells (1 / 0).
 * scratch: dvq_attn_causal_scratch_bytes(B, T, 1, C, backward) bytes (forward: 0, NULL). */
int dvq_attn_full_ok(int dtype, int64_t B, int64_t T, int C);
int dvq_attn_full_fwd(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int C, float scale, void* out,
                      float* lse, void* scratch, dvq_stream_t stream);
int dvq_attn_full_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, int dtype,
                      int64_t B, int64_t T, int C, float scale, void* dq, void* dk, void* dv, void* scratch, dvq_stream_t stream);
/* Attention of ONE new query row per sequence over a K/V cache (KV-cached sampling; the reference's sampler recomputes the
 * whole prefix, stackgpt.py:234-339): q [B][C], kcache / vcache [B][Tmax][C] (C = n_head * head_size), T valid rows incl.
 * the new one; out [B][C] = softmax(scale * q K^T) V per head. */
int dvq_attn_decode(const void* q, const void* kcache, const void* vcache, int dtype, int64_t B, int64_t n_head, int64_t head_size,
                    int64_t T, int64_t Tmax, float scale, void* out, dvq_stream_t stream);
/* Device-indexed forms for a captured hipGraph (one graph replayed for every sampled token): the cache row index t is read
 * from device memory.  dvq_attn_decode_dev stores k_new / v_new [B][C] into cache row t and attends over rows [0, t];
 * dvq_rows_dev copies x [B][C] into hidden[b][t][:] (store != 0) or back.  Calls with t outside [0, Tmax) do nothing. */
int dvq_attn_decode_dev(const void* q, const void* k_new, const void* v_new, void* kcache, void* vcache, int dtype, int64_t B,
                        int64_t n_head, int64_t head_size, const int64_t* t_dev, int64_t Tmax, float scale, void* out,
                        dvq_stream_t stream);
int dvq_rows_dev(void* x, void* hidden, int dtype, int64_t B, int64_t C, int64_t Tmax, const int64_t* t_dev, int store,
                 dvq_stream_t stream);

/* One token step of ALL blocks of a StackGPT transformer (stackgpt.py:41-96 Block / CausalSelfAttention, one new row per sequence
 * against K/V caches) as ONE persistent kernel: per block LayerNorm + q / k / v (k, v appended to the caches at row t_dev[0]),
 * single-row attention per (sequence, head), projection + residual, LayerNorm + fc + GELU, projection + residual -- the phases
 * separated by a device-wide barrier.  Replaces 12 launches per block of the K/V-cached sampler (each costs ~9 us of command
 * processing whatever its size).  bf16 weights [out][in] (row-major, as torch.nn.Linear), fp32 biases (may be NULL) and LayerNorm
 * parameters; B <= 64 sequences, C %% 32 == 0 (<= 2048), F %% 32 == 0, head size %% 8 == 0; x [B][C] bf16 is updated in place.
 * `layers_dev`: DEVICE array of n_layers dvq_decode_layer.  `scratch`: dvq_decode_stack_scratch_bytes(B, C, F) bytes, ZEROED once by
 * the caller (the kernel re-arms its barrier counters itself).  n_workgroups <= 0: one workgroup per CU; the grid must be resident
 * as a whole (nothing else may occupy the device's LDS / wave slots to the point of excluding a workgroup: a barrier that is not
 * reached within seconds sets the error word and releases every workgroup, all of which leave the kernel -- read it with
 * dvq_decode_stack_status -- instead of hanging or continuing on stale data).
 * The buffers the phases exchange are accessed with agent-scope atomics (memory side): the barrier needs no cache flush.
 * Round 4, the default for B <= 16: the same five phases as FIVE LAUNCHES per block (DVQ_DECODE_MODE=phases / persistent): a dependent
 * kernel boundary costs 1.2 - 1.9 us on this chip, a 128-workgroup barrier plus the memory-side exchange 6 - 9 us per phase.
 * `layers_host` (may be NULL): a HOST copy of the same array; the phase launches then carry each block's pointers by value instead
 * of starting with a dependent load of the device table. */
typedef struct dvq_decode_layer {
    const void *wq, *wk, *wv, *wo, *w1, *w2;          /* bf16 [C][C] x 4, [F][C], [C][F] */
    const float *bq, *bk, *bv, *bo, *b1, *b2;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    void *kcache, *vcache;                            /* bf16 [B][Tmax][C] */
} dvq_decode_layer;
size_t dvq_decode_stack_scratch_bytes(int64_t B, int64_t C, int64_t F);
/* 1 when dvq_decode_stack takes this geometry (its own shape check), else 0: the caller keeps the per-kernel token steps */
int dvq_decode_stack_ok(int64_t B, int64_t C, int n_head, int64_t F, int64_t Tmax);
/* Synchronising read-back of the error word of dvq_decode_stack (call once per sampling run, not per token): DVQ_OK, or
 * DVQ_ELAUNCH when a device-wide barrier timed out since the scratch was last zeroed -- every workgroup left the kernel at that
 * barrier, so the rows produced since are invalid; reset != 0 re-arms the counters (on `stream`) so that later launches run. */
int dvq_decode_stack_status(const void* scratch, int64_t B, int64_t C, int64_t F, int reset, dvq_stream_t stream);
int dvq_decode_stack(const void* layers_dev, int n_layers, int64_t B, int64_t C, int n_head, int64_t F, int64_t Tmax, const int64_t* t_dev,
                     float eps, void* x, void* scratch, int n_workgroups, const void* layers_host, dvq_stream_t stream);
/* nn.Dropout(p) with a counter-based hash RNG: y = x * keep / (1-p); the same (seed) reproduces the mask for the backward */
int dvq_dropout(const void* x, int dtype, int64_t n, float p, uint64_t seed, void* y, dvq_stream_t stream);
/* y = x + dropout(a), the decisions of dvq_dropout for the same seed (p = 0: y = x + a): residual add + resid_drop of a block in one pass */
int dvq_dropout_add(const void* x, const void* a, int dtype, int64_t n, float p, uint64_t seed, void* y, dvq_stream_t stream);
/* Label dropout of classifier-free-guidance training: out[i] = null_label where dvq_dropout's keep hash of (seed, element i) drops
 * element i (probability p, 0 <= p <= 1; p = 1 drops every label), else labels[i].  labels, out: int64 [B] (may alias) */
int dvq_label_dropout(const int64_t* labels, int64_t B, float p, int64_t null_label, uint64_t seed, int64_t* out, dvq_stream_t stream);

/* AdamW step whose hyper-parameters are read from DEVICE memory (so that a step captured as a hipGraph follows the LR schedule):
 * hyper[8] = {lr / (1 - beta1^t), beta1, beta2, eps, 1 / sqrt(1 - beta2^t), 1 - lr * weight_decay, unused, unused}.
 * Same update as dvq_adamw (models/stage1_dynamic/dqvae_dual_entropy.py:228-232 Adam, dqtransformer_uncond_entropy.py:92-128 AdamW). */
int dvq_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, dvq_stream_t stream);
/* Global gradient norm of one optimizer's flat gradient buffer, with the clip coefficient of torch.nn.utils.clip_grad_norm_ and a
 * finite flag (Lightning's --gradient_clip_val, applied once per optimizer; docs/design/19-gradient-clipping.md).  Two launches, no
 * atomics, no host read: (1) one fp64 partial of sum g^2 per fixed 32768-element chunk into `workspace`
 * (dvq_grad_sqnorm_workspace_bytes(n), caller-owned), (2) one workgroup adds the partials in a fixed order and writes
 *   gstat (32 bytes, 8-byte aligned) = { double norm = sqrt(sum g^2);
 *                                        float coef = clip > 0 ? min(1, clip / (norm + 1e-6)) : 1;
 *                                        int32 finite = isfinite(sum g^2);
 *                                        int32 skipped += (skip_nonfinite && !finite);     running count, never reset here
 *                                        int32 skip = (skip_nonfinite && !finite);         read by dvq_adamw_clip_dev
 *                                        float clip; int32 skip_nonfinite }                echo of the arguments
 * The order of every addition depends on n alone: equal buffers give bit-equal results on every device and every launch.  Squares
 * are taken in fp64, so `finite` is false iff an element is Inf / NaN.  clip must be finite and >= 0 (0 = no clipping). */
size_t dvq_grad_sqnorm_workspace_bytes(int64_t n);
int dvq_grad_sqnorm(const float* g, int64_t n, float clip, int skip_nonfinite, void* workspace, size_t workspace_bytes,
                    void* gstat, dvq_stream_t stream);
/* dvq_adamw_dev on the gradient g * gstat.coef (g is not rewritten); returns without touching p, m, v when gstat.skip is set.
 * With coef == 1 the results are bit-identical to dvq_adamw_dev. */
int dvq_adamw_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, const void* gstat,
                       dvq_stream_t stream);
/* Weight EMA (shadow weights for evaluation, tf.train.ExponentialMovingAverage / taming's LitEma; docs/design/20-weight-ema.md):
 *   e[i] <- e[i] - om * (e[i] - p[i]),  om = rec[0] = 1 - decay of this step, READ FROM DEVICE MEMORY (rec: 8 floats, [0] used), so a
 * step captured as a hipGraph replays with the decay of the current step.  The host forms 1 - decay in fp64 and rounds it once.
 * gstat: NULL, or the statistics block of dvq_grad_sqnorm -- when its skip field is set the kernel returns before touching memory,
 * like dvq_adamw_clip_dev.  16-byte accesses when e and p are both 16-byte aligned, 4-byte ones otherwise.  No atomics; equal
 * inputs give bit-equal outputs on every launch; p == e leaves e bit for bit.  e and p must not overlap. */
int dvq_ema_update(float* e, const float* p, int64_t n, const float* rec, const void* gstat, dvq_stream_t stream);
/* exchange the contents of two non-overlapping fp32 buffers in one launch, without a third buffer (overlap: DVQ_EINVAL) */
int dvq_swap_f32(float* a, float* b, int64_t n, dvq_stream_t stream);
/* Per-segment statistics of a flat fp32 buffer -- per-parameter gradient, weight and update norms (Lightning's --track_grad_norm;
 * docs/design/24-norm-tracking.md).  The buffer [0, n) is cut into S back-to-back segments by S + 1 ascending element offsets
 * (offsets[0] = 0, offsets[S] = n, every length >= 1); the element value is a[i], or with b != NULL (double)a[i] - (double)b[i].
 * The ordered two-stage form of dvq_grad_sqnorm, segmented: every segment is cut into chunks of 32768 elements (the last one shorter),
 * (1) one workgroup per chunk stores one partial into `workspace` with plain stores, (2) one wave per segment adds that segment's
 * partials in index order and writes the segment's row of
 *   state = { double sumsq[S]            sum of v^2 over the finite elements, squares in fp64;
 *             int64  nonfinite[S]        Inf / NaN elements of THIS launch (with b: either operand), left out of the other two;
 *             int64  nonfinite_total[S]  sticky: += nonfinite;
 *             int64  first_bad_call[S]   sticky: the launch counter at the first launch with nonfinite != 0, -1 before (set by the caller);
 *             int64  calls[S]            sticky: the launch counter, one copy per segment, += 1 per launch;
 *             float  absmax[S] }         max |v| over the finite elements, rounded to fp32
 * (dvq_segment_stats_state_bytes(S) bytes, 8-byte aligned; the caller zeroes it and sets first_bad_call to -1 before the first launch).
 * sticky == 0 leaves the three sticky arrays untouched.  No atomics; the order of every addition depends on the offsets alone: equal
 * inputs give bit-equal state on every launch, whatever the alignment of a and b (16-byte loads where a chunk starts on a 16-byte
 * boundary, 4-byte loads elsewhere, the same element-to-accumulator assignment in both).  Never counted as an unordered launch.
 * The chunk table lives in device memory: dvq_segment_plan_build writes the plan (the offsets, each segment's first chunk, one
 * {start, segment, length} record per chunk) into HOST memory, dvq_segment_plan_bytes(offsets, S, n) bytes (0 for a bad table); the
 * caller copies it to the device once.  `offsets` is a HOST pointer in all three calls: dvq_segment_stats checks it on every call
 * (DVQ_ESHAPE for a table that is not ascending from 0 to n, or a plan whose size does not belong to it; DVQ_EWORKSPACE for a
 * workspace below dvq_segment_stats_workspace_bytes(n, S)) before it launches anything; that plan_dev holds the plan built from the same
 * offsets is the caller's contract.
 * armed: NULL, or a device int32 -- when it is 0 both kernels return before touching any other memory (one wave-uniform load, like the
 * skip flag of dvq_adamw_clip_dev), so a recorded step carries the launches and only row steps pay for them. */
size_t dvq_segment_stats_workspace_bytes(int64_t n, int64_t S);
size_t dvq_segment_stats_state_bytes(int64_t S);
size_t dvq_segment_plan_bytes(const int64_t* offsets, int64_t S, int64_t n);
int dvq_segment_plan_build(const int64_t* offsets, int64_t S, int64_t n, void* plan_host, size_t plan_host_bytes);
int dvq_segment_stats(const float* a, const float* b, int64_t n, const int64_t* offsets, int64_t S, const void* plan_dev,
                      size_t plan_bytes, void* workspace, size_t workspace_bytes, void* state, int sticky, const int* armed,
                      dvq_stream_t stream);
/* dst[i] <- src[i], 16-byte accesses when both are 16-byte aligned; returns at once when armed != NULL and *armed == 0 (the snapshot
 * of the parameters in front of Adam on row steps) */
int dvq_copy_f32_armed(float* dst, const float* src, int64_t n, const int* armed, dvq_stream_t stream);
/* dst[0..7] <- the eight scalars (passed by value in the launch: no pageable host copy, no host buffer to keep alive) */
int dvq_set_f32x8(float* dst, float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7,
                  dvq_stream_t stream);
/* Training metric logs (docs/design/22-metrics-logging.md).
 * dvq_scalar_push gathers `count` <= 64 scalars into columns col0 .. col0 + count - 1 of a caller-owned state block of `columns` <= 256
 * columns (dvq_scalar_push_state_bytes(columns) bytes, 8-byte aligned, zeroed by the caller before the first push and whenever the
 * running sums restart):
 *   state = { double sum[columns]; int64 cnt[columns]; int64 bad[columns]; float last[columns] }
 * Scalar i is described BY VALUE in the record: code[i] one of DVQ_SCALAR_*, addr[i] the device address of one element of that type
 * (naturally aligned), or for DVQ_SCALAR_IMM the value itself as the bit pattern of a double.  The record is copied into the launch
 * arguments: the caller may free it at once, a recorded step keeps its own copy, no device pointer table exists.  Each value v is read
 * once; column c = col0 + i then gets
 *   last[c] = (float)v;   v finite: sum[c] += (double)v, cnt[c] += 1;   else: bad[c] += 1.
 * One workgroup, one owner thread per column, no atomics: the order of the additions into a column is the order of the launches, equal
 * inputs give bit-equal state, and the launch is not counted as unordered.  More than 64 scalars: several launches with rising col0.
 * columns outside 1 .. 256, count outside 1 .. 64 or col0 + count > columns: DVQ_ESHAPE; the state_bytes call returns 0 then. */
enum { DVQ_SCALAR_F32 = 0, DVQ_SCALAR_BF16 = 1, DVQ_SCALAR_F64 = 2, DVQ_SCALAR_I32 = 3, DVQ_SCALAR_I64 = 4, DVQ_SCALAR_IMM = 5,
       DVQ_SCALAR_SKIP = 6 /* no scalar for this column in this launch: the column is left untouched */ };
enum { DVQ_SCALAR_PUSH_MAX = 64, DVQ_SCALAR_COLUMNS_MAX = 256 };
typedef struct {
    uint64_t addr[64]; /* DVQ_SCALAR_PUSH_MAX device addresses (DVQ_SCALAR_IMM: fp64 bits of the value) */
    uint8_t code[64];  /* DVQ_SCALAR_* of each */
} dvq_scalar_record;
size_t dvq_scalar_push_state_bytes(int64_t columns);
int dvq_scalar_push(const dvq_scalar_record* rec, int32_t count, int32_t col0, int32_t columns, void* state, dvq_stream_t stream);
/* Codebook usage of one step from per-code counts n[k] = counts[k * stride], k < K; counts_type DVQ_SCALAR_F32 or DVQ_SCALAR_I64 (the
 * EMA quantiser's counts are column D of its fp32 [K, D + 1] statistics: stride D + 1).  Writes
 *   out3 = { perplexity exp(-sum p log p) with p = n / sum n over the codes with n > 0;  number of codes with n > 0;  sum n }
 * as fp32, computed in fp64 (out3_f64: NULL or three doubles that receive the same values before that rounding); sum n == 0 gives
 * perplexity 0 and 0 active codes.  total: NULL or double [K], total[k] += n[k] (running usage of an epoch).  One workgroup; thread t
 * owns the codes k = t mod 256 in ascending order, the 256 partials meet in a fixed tree: no atomics, bit-equal for equal inputs. */
int dvq_codebook_health(const void* counts, int counts_type, int64_t K, int64_t stride, float* out3, double* out3_f64, double* total,
                        dvq_stream_t stream);
/* k distinct pseudo-random indices in [0, n) = prefix of a keyed Feistel permutation (replaces torch.randperm(n)[:k] of
 * quantize2_mask.py:93-98); state = uint64[2] {seed, counter} in device memory, the counter is advanced on the stream. */
int dvq_sample_rows(int64_t* out, int64_t k, int64_t n, uint64_t* state, dvq_stream_t stream);
/* x[i] += scale * U[0,1), fp32, same state convention (the noise of _tile_with_noise, quantize2_mask.py:57-64: torch.rand_like
 * under stream capture depends on torch's graph executor rewriting the Philox offset, which a launch-list replay does not run) */
int dvq_add_uniform(float* x, int64_t n, float scale, uint64_t* state, dvq_stream_t stream);

int dvq_fill_f32(float* p, float v, int64_t n, dvq_stream_t stream);

/* ---- input pipeline (data/imagenet_base.py:16-32: Resize(256) -> Random/CenterCrop(256) -> RandomHorizontalFlip -> ToTensor ->
 * Normalize(0.5, 0.5)) on DECODED uint8 RGB images of one batch.  `src`: the images packed back to back ([h][w][3] each);
 * `desc`: B records of dvq_image_desc_bytes() bytes (layout: ImgDesc in csrc/imgproc.hip, mirrored by data._Desc) giving per
 * image its size, crop window in the resized image, flip flag, the input-row window of the vertical pass and offsets into
 * `tables` (Pillow's antialiased-bilinear bounds + 22-bit fixed-point coefficients, computed by the caller for the crop's columns
 * and rows only); `tmp`: scratch for the horizontally resampled rows; `out`: fp32 [B][3][S][S] in [-1, 1].  Bit-exact with
 * Pillow 9.4 / torchvision 0.14 on the same decoded pixels. */
size_t dvq_image_desc_bytes(void);
int dvq_image_batch_transform(const uint8_t* src, const void* desc, const int32_t* tables, uint8_t* tmp, int64_t B, int S,
                              int max_rows, float* out, dvq_stream_t stream);

/* ---- device JPEG decode (docs/design/23-device-jpeg.md): the Huffman pass on the host, everything after the coefficients on the GPU,
 * pixel for pixel what libjpeg-turbo's default path gives (integer "islow" IDCT, fancy upsampling, fixed-point colour).
 *
 * Host pass (csrc/jpeg_host.cpp: no GPU, no allocation, no state; safe to call from many threads on any bytes).
 * dvq_jpeg_info parses the markers up to the first SOS and fills `info`.  info->supported is DVQ_JPEG_SUPPORTED for what the decoder
 * takes: 8-bit baseline or extended-sequential Huffman (SOF0 / SOF1), one interleaved scan, 1 component or 3 (YCbCr) with luma sampling
 * 1x1, 2x1 or 2x2 over 1x1 chroma; otherwise the reason, and the caller decodes the file some other way.  Returns DVQ_EINVAL only for
 * null pointers.
 * dvq_jpeg_entropy_decode byte-unstuffs and Huffman-decodes every MCU of a supported stream (restart markers included):
 *   coef  int16 [component][block_row][block_col][64], natural (de-zigzagged) order, NOT dequantised, the block grid of each component
 *         padded to whole MCUs; info->coef_count elements (coef_capacity smaller: DVQ_EWORKSPACE)
 *   qtab  uint16 [component][64], natural order: the quantisation table of each component
 * A stream that is unsupported, malformed or ends early returns DVQ_EINVAL with the message in dvq_last_error; it never reads outside
 * [data, data + n) and never writes past coef_capacity. */
enum {
    DVQ_JPEG_SUPPORTED = 0,
    DVQ_JPEG_NOT_JPEG = 1,     /* no SOI at the start */
    DVQ_JPEG_MALFORMED = 2,    /* markers cut short or inconsistent, tables missing, dimensions of 0 */
    DVQ_JPEG_PROGRESSIVE = 3,  /* SOF2 */
    DVQ_JPEG_ARITHMETIC = 4,   /* SOF9 .. SOF15 */
    DVQ_JPEG_SOF_KIND = 5,     /* lossless or hierarchical frames */
    DVQ_JPEG_PRECISION = 6,    /* not 8 bits per sample */
    DVQ_JPEG_COMPONENTS = 7,   /* neither 1 nor 3 components (CMYK, YCCK) */
    DVQ_JPEG_SAMPLING = 8,     /* a sampling grid other than 1x1, 2x1, 2x2 luma over 1x1 chroma */
    DVQ_JPEG_COLORSPACE = 9,   /* 3 components that are not YCbCr (Adobe transform 0, or ids R G B without JFIF) */
    DVQ_JPEG_MULTISCAN = 10    /* the first scan does not hold every component */
};
typedef struct dvq_jpeg_info_t {
    int32_t width, height, components, restart_interval;
    int32_t h_samp[4], v_samp[4], qtab_index[4]; /* per component; a one-component stream reports 1x1 */
    int32_t supported;                           /* DVQ_JPEG_* */
    int32_t reserved;
    int64_t coef_count;                          /* int16 elements dvq_jpeg_entropy_decode writes; 0 unless supported */
} dvq_jpeg_info_t;
int dvq_jpeg_info(const uint8_t* data, size_t n, dvq_jpeg_info_t* info);
int dvq_jpeg_entropy_decode(const uint8_t* data, size_t n, int16_t* coef, int64_t coef_capacity, uint16_t* qtab);
/* Device stage (csrc/jpeg.hip), two launches for a whole batch of differently sized images:
 *   (a) dequantise, 8x8 inverse DCT, + 128, clamp -> uint8 component planes in planes_tmp (each plane as large as its padded block grid)
 *   (b) fancy chroma upsampling on the unpadded chroma planes, YCbCr -> RGB, packed uint8 [h][w][3] at each image's offset in rgb_out
 *       (a one-component image writes its sample to all three channels)
 * coef: the batch's coefficients back to back (device); desc: B records of dvq_jpeg_desc_bytes() bytes in device memory (layout: JpegDesc
 * in csrc/jpeg.hip, mirrored by data._JpegDesc) with per image its offsets into coef, planes_tmp and rgb_out, size, sampling, tables and
 * its share of the two grids; a record with 0 components is skipped (its slot in rgb_out is the caller's to fill).  rgb_out is what
 * dvq_image_batch_transform reads as `src`. */
size_t dvq_jpeg_desc_bytes(void);
int dvq_jpeg_batch_decode(const int16_t* coef, const void* desc, int64_t B, uint8_t* planes_tmp, uint8_t* rgb_out, dvq_stream_t stream);

/* ---- device PNG decode (docs/design/29-device-png.md): the host parses the chunks, checks the CRCs and inflates the IDAT stream
 * (data.decode_png_host, pure Python over zlib); the device reverses the PNG filters (None, Sub, Up, Average, Paeth) of a whole batch of
 * differently sized images in one launch (csrc/png.hip), pixel for pixel what PIL decodes.
 * scan: the batch's FILTERED scanlines back to back (device), per image h rows of 1 filter byte (0..4, checked by the host) and w * bpp
 * bytes; desc: B records of dvq_png_desc_bytes() bytes in device memory (layout: PngDesc in csrc/png.hip, mirrored by data._PngDesc)
 * with per image scan_off, rgb_off, w, h and bpp (1 grey, 2 grey + alpha, 3 RGB, 4 RGBA; 8 bits per sample).  Output per image: packed
 * uint8 [h][w][3] at rgb_off of rgb_out, grey written to all three channels, alpha dropped; no byte outside the images' slots is
 * written.  rgb_out is what dvq_image_batch_transform reads as `src`, and the buffer dvq_jpeg_batch_decode fills. */
size_t dvq_png_desc_bytes(void);
int dvq_png_batch_unfilter(const uint8_t* scan, const void* desc, int64_t B, uint8_t* rgb_out, dvq_stream_t stream);

/* ---- reconstruction evaluation (no reference kernel: its codebook-usage tool collects codes on the host,
 * scripts/tools/codebook_usage_dqvae.py:52-69; SSIM as Wang et al. 2004) -----------------------------------------------------------
 * dvq_recon_metrics: x (target), y (reconstruction) NCHW fp32 [B][3][H][W] in [-1, 1]; per image fp64 outputs
 *   mse[b]  = mean over 3 H W of (x01 - y01)^2, v01 = clamp(v * 0.5 + 0.5, 0, 1), with quantize_u8 = 1 then floor(v01 * 255 + 0.5) / 255
 *             (the value a saved 8-bit PNG holds);
 *   l1[b]   = mean of |x - y| on the raw inputs ([-1, 1] units, the units of the training loss's L1 term; neither clamped nor quantised);
 *   ssim[b] = mean over the 3 channels and the (H - 10) x (W - 10) "valid" positions of the SSIM map of x01 / y01: 11 x 11 Gaussian
 *             window (sigma 1.5, normalised), C1 = 0.01^2, C2 = 0.03^2, population (biased) variances.
 * H < 11 or W < 11: DVQ_ESHAPE.  ws: dvq_recon_metrics_workspace_bytes(B, H, W) bytes (per-tile partial sums; ws_bytes smaller:
 * DVQ_EWORKSPACE).  Partials are folded per image in a fixed order (no float atomics): the outputs are bitwise reproducible and
 * independent of how images are grouped into batches.
 * dvq_code_histogram: idx int64 [B][Hf][Wf] (VectorQuantize2's code map), grain int64 [B][hg][wg] (0 = coarsest) or NULL with G = 1.
 *   Position (i, j) is a token iff i % s == 0 && j % s == 0, s = (Hf / hg) >> grain[i / (Hf / hg)][j / (Wf / wg)], with
 *   Hf / hg == Wf / wg == 2^(G-1) (else DVQ_ESHAPE): a cell of grain g spends 4^g tokens; grain = NULL: every position is a token.
 *   counts int64 [G][K] += tokens per (grain, code) (the caller zeroes it once; accumulates over calls); tokens int64 [B] = tokens per
 *   image (overwritten; a token whose code is out of range still counts); invalid int64 [1] += codes outside [0, K) at token positions
 *   + grain cells whose value is outside [0, G) (such a cell spends no token).  Integer atomics only: exact and deterministic.
 * dvq_recon_cells (docs/design/30-cell-maps.md): the same pair of images cut into an hg x wg grid of (H / hg) x (W / wg) pixel cells,
 *   H % hg == 0 and W % wg == 0 (else DVQ_ESHAPE; any H, W >= 1).  cells fp64 [B][hg][wg][3], per cell and summed over the 3 channels:
 *   [0] sum over the cell's pixels of (x01 - y01)^2, [1] sum of |x - y| on the raw values, [2] sum of the SSIM index over the valid
 *   11 x 11 windows whose TOP-LEFT pixel lies in the cell (a window at (r, c) is valid iff r <= H - 11 and c <= W - 11; a cell without
 *   one reports 0, and the caller derives the window count from the geometry).  Same x01, staging (v01 - 0.5), fp32 moments and fp64
 *   error terms as dvq_recon_metrics; sums are NOT divided.  ws: dvq_recon_cells_workspace_bytes(B, H, W, hg, wg) bytes (0 for a bad
 *   grid).  Every partial sum has one owner and a fixed order: two launches give the same bits and an image's map does not depend on
 *   its batch.  dvq_recon_metrics is untouched by it. */
size_t dvq_recon_metrics_workspace_bytes(int64_t B, int64_t H, int64_t W);
int dvq_recon_metrics(const float* x, const float* y, int64_t B, int64_t H, int64_t W, int quantize_u8, double* mse, double* l1,
                      double* ssim, void* ws, size_t ws_bytes, dvq_stream_t stream);
int dvq_code_histogram(const int64_t* idx, const int64_t* grain, int64_t B, int64_t Hf, int64_t Wf, int64_t hg, int64_t wg, int64_t K,
                       int G, int64_t* counts, int64_t* tokens, int64_t* invalid, dvq_stream_t stream);
size_t dvq_recon_cells_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t hg, int64_t wg);
int dvq_recon_cells(const float* x, const float* y, int64_t B, int64_t H, int64_t W, int64_t hg, int64_t wg, int quantize_u8,
                    double* cells, void* ws, size_t ws_bytes, dvq_stream_t stream);

/* ---- likelihood scoring of the DQ-Transformer (docs/design/15-likelihood.md; no reference kernel: it logs batch-mean losses only) ------
 * dvq_token_nll: logits [rows][ldl] of `dtype`, the first V columns are used (columns V .. ldl are padding and never enter a result);
 *   target int64 [rows].  Per row, in fp32 with the maximum subtracted and the natural logarithm:
 *   nll[r]  = log(sum_{c < V} exp(x[c] - max)) - (x[target] - max);
 *   rank[r] = #{c < V : x[c] > x[target]} + #{c < target : x[c] == x[target]}  (0 = the target is the top-1 guess; ties go to the
 *             lower column index, the order of a stable descending sort);
 *   target[r] == ignore_index: nll = 0, rank = -1.  Any other target outside [0, V): nll = NaN, rank = V (no column is read for it).
 *   -inf logits in other columns contribute 0.  Each row is read once (plus one re-read of x[target] when the rows are not 16-byte
 *   aligned or V > 2048) and written by one lane: no atomics, no [rows, V] temporary, bitwise reproducible.  Any V >= 1.
 * dvq_nll_segment_sums: rows laid out [B][Tp]; out fp64 [B][2][4] = (sum of nll, tokens, top-1 hits (rank == 0), top-5 hits
 *   (rank < 5)) over the rows with rank >= 0 of segment 0 = [0, split) and segment 1 = [split, Tp), 0 <= split <= Tp.  One workgroup per
 *   (image, segment), fixed summation order in fp64: two launches on the same input give the same bits.
 * dvq_nll_cell_sums (docs/design/30-cell-maps.md): the same rows and segments keyed by grid cell.  pos int64 [B][Tp]: the position code
 *   that decides a row's cell -- a COARSE code in segment 0 (code p in [0, hw1^2) is cell p), a FINE code in segment 1 (code e in
 *   [0, (hw1 hw2)^2) is cell (e / fhw / hw2) * hw1 + (e % fhw) / hw2, fhw = hw1 * hw2: the cell dvq_permute_dual_back writes position
 *   e into).  A row with rank >= 0 whose code is no grid position adds to `outside`; rows with rank < 0 add nothing.  Segment s is
 *   written to stream index stream_s in [0, 4) of cells fp64 [B][4][hw1^2][4] and outside fp64 [B][4][4] (same four values as
 *   dvq_nll_segment_sums); stream_s = -1 skips the segment and leaves its outputs alone.  One owner thread per output cell walks the
 *   rows in row order: no atomics, bitwise reproducible. */
int dvq_token_nll(const void* logits, int dtype, int64_t rows, int64_t V, int64_t ldl, const int64_t* target, int64_t ignore_index,
                  float* nll, int32_t* rank, dvq_stream_t stream);
int dvq_nll_segment_sums(const float* nll, const int32_t* rank, int64_t B, int64_t Tp, int64_t split, double* out, dvq_stream_t stream);
int dvq_nll_cell_sums(const float* nll, const int32_t* rank, const int64_t* pos, int64_t B, int64_t Tp, int64_t split, int hw1, int hw2,
                      int stream0, int stream1, double* cells, double* outside, dvq_stream_t stream);

/* ---- token shards (docs/design/16-token-shards.md; no reference kernel: the reference re-encodes every image in every stage-2 step) ---
 * dvq_tokens_pack: indices int64 [B][fhw][fhw], grain int64 [B][hw1][hw1] (what DualGrainVQModel.encode returns; fhw = hw1 * hw2) ->
 *   codes u16 [B][fhw * fhw]; grain_bits u32 [B][W], W = ceil(hw1^2 / 32): bit c % 32 of word c / 32 is 1 iff cell c (row-major) is fine,
 *   bits past the grid are 0; n_fine_cells int32 [B]; bad int32 [B] = codes outside [0, min(codebook_size, 65536)) + grain values other
 *   than 0 / 1 of image b.  Such an image is still written: its codes are clamped into the range, a bad grain value counts as coarse.
 * dvq_tokens_unpack: codes / grain_bits as above -> the four rows of dvq_permute_dual (same pad / eos arguments, order 0 region-first,
 *   1 row-first with ANY hw2) at the caller's row lengths: coarse_content / coarse_position int64 [B][Lc], fine_content / fine_position
 *   int64 [B][Lf], EOS-terminated and PAD-filled.  With Lc = max_b(coarse cells) + 1 and Lf = max_b(fine codes) + 1 they equal
 *   DualGrainSeperatePermuter.forward's output bit for bit; larger lengths add padding; a row that does not fit is cut at Lc / Lf
 *   (nothing is written beyond them).  Bits of grain_bits past the grid are ignored.  hw1^2 > 1024: DVQ_ESHAPE. */
int dvq_tokens_pack(const int64_t* indices, const int64_t* grain, int64_t B, int hw1, int hw2, int64_t codebook_size, uint16_t* codes,
                    uint32_t* grain_bits, int32_t* n_fine_cells, int32_t* bad, dvq_stream_t stream);
int dvq_tokens_unpack(const uint16_t* codes, const uint32_t* grain_bits, int64_t B, int hw1, int hw2, int order, int64_t content_pad,
                      int64_t content_eos, int64_t cpos_pad, int64_t cpos_eos, int64_t fpos_pad, int64_t fpos_eos, int64_t Lc, int64_t Lf,
                      int64_t* coarse_content, int64_t* coarse_position, int64_t* fine_content, int64_t* fine_position,
                      dvq_stream_t stream);

/* ---- gradient-trained codebook (MaskVectorQuantize, quantize_codebook_mask.py) -- csrc/vq_trained.hip ----------------------------
 * Prepared codebook of dvq_vq_sample_argmax: two bf16 planes (e = e1 + e2 to 2^-17) and a per-code bias; cosine != 0 stores the rows
 * normalised (e / max(|e|, 1e-12)) with bias 0, else the raw rows with bias -|e_k|^2.  Rebuild it whenever the codebook changes. */
size_t dvq_vq_trained_prep_bytes(int64_t K, int64_t D);
int dvq_vq_trained_prepare(const float* codebook, int64_t K, int64_t D, int cosine, void* prep, dvq_stream_t stream);
/* idx[n] = argmax_k (s[n,k] / temp + g(n,k)), lowest index on ties, never forming [N,K].  s = -|x_n - e_k|^2 (cosine == 0) or the cosine
 * similarity of x_n and e_k (`cosine` must match the prepare call); g = -log(-log(u)) Gumbel noise from a counter-based hash of
 * (seed, draw counter, n, k).  temp == 0: no noise (plain argmax of s; `state` may be NULL).  temp > 0: state = uint64[2] {seed, counter}
 * in device memory, the counter is advanced by ONE on the stream after the search (replays of a recorded step draw fresh noise).
 * x: [N,D] fp32 or bf16.  D in {64, 128, 256}: bf16 MFMA with split operands (x1.e1 + x1.e2 + x2.e1, fp32 accumulate; bf16 rows:
 * two products); every other D <= 4096: a plain kernel.  N < 2^31, K < 2^24.  With noise there is no re-rank: scores closer than the
 * evaluation error (~3 * 2^-18 |x||e| / temp) may resolve either way.  The noiseless COSINE search (cosine != 0, temp == 0) is exact:
 * rows whose two best scores are within the evaluation bound are re-ranked in fp64 from `codebook` (the raw fp32 [K,D] rows the
 * prepare call saw; required in that case, else it may be NULL).  The noiseless L2 form is not re-ranked: dvq_vq_argmin is the exact one. */
int dvq_vq_sample_argmax(const void* x, int x_dtype, const void* prep, const float* codebook, int64_t N, int64_t K, int64_t D, int cosine,
                         float temp, uint64_t* state, int64_t* idx, dvq_stream_t stream);
/* out[n,k] = g(n,k) of the draw (seed, counter): the noise dvq_vq_sample_argmax adds when its state holds these two values.
 * fp32 [N,K]; tests and analysis only. */
int dvq_vq_gumbel_noise(uint64_t seed, uint64_t counter, int64_t N, int64_t K, float* out, dvq_stream_t stream);
/* grad[k,:] += coef_dev[0] * sum_{n: idx[n] = k} mask[n] * (codebook[k,:] - x[n,:])   (mask NULL = 1).  grad: fp32 [K,D], accumulated.
 * One wave per (code, slice of 1024 rows) + fp32 atomics; under dvq_set_deterministic(1) one wave per code walks all rows in order
 * and adds without atomics: repeated launches are bit-identical. */
int dvq_vq_codebook_grad(const void* x, int dtype, const float* codebook, const int64_t* idx, const float* mask, const float* coef_dev,
                         int64_t N, int64_t K, int64_t D, float* grad, dvq_stream_t stream);
/* out[0] = N / sum(mask) (fp32; one workgroup, fixed order): the loss' mask-ratio normalisation without a host read */
int dvq_vq_mask_ratio(const float* mask, int64_t N, float* out, dvq_stream_t stream);
/* Orthogonality regulariser sum((W W^T - I)^2), W = normalize(E), around the caller's two GEMMs:
 * rownorm: w[k,:] = e[k,:] * inv[k], inv[k] = 1 / max(|e[k,:]|, 1e-12);  ortho_sumsq: g [K,K] -= I in place, out[0] = scale * sum(g^2)
 * (scratch: dvq_vq_ortho_scratch_bytes());  rownorm_bwd: grad[k,:] += coef_dev[0] * scale * inv[k] * (dw[k,:] - w[k,:] (w[k,:] . dw[k,:])) */
int dvq_vq_rownorm(const float* e, int64_t K, int64_t D, float* w, float* inv, dvq_stream_t stream);
size_t dvq_vq_ortho_scratch_bytes(void);
int dvq_vq_ortho_sumsq(float* g, int64_t K, float scale, void* scratch, float* out, dvq_stream_t stream);
int dvq_vq_rownorm_bwd(const float* w, const float* inv, const float* dw, const float* coef_dev, float scale, int64_t K, int64_t D,
                       float* grad, dvq_stream_t stream);

/* ---- training-time image logging (csrc/imagelog.hip, docs/design/18-image-logging.md) ----------------------------------------------
 * The reference's panels and grid (modules/dynamic_modules/utils.py:41-161, utils/logger.py:137-147) computed on the device.  Every
 * value is fp32 IEEE, each product / sum / quotient rounded on its own, true divisions, float -> byte conversions truncate; the only
 * reductions are minima and maxima: outputs are bitwise reproducible.  Inputs are expected finite.
 * ws: dvq_imagelog_workspace_bytes(segments) bytes of partial extrema, segments = B for the overlay, 1 for the grid (smaller:
 * DVQ_EWORKSPACE).  Tensors of 2^31 elements or more are refused (DVQ_ESHAPE).
 *
 * dvq_grain_overlay: x fp32 NCHW [B][3][H][W]; EITHER grain int64 [B][h][w] with levels in {2, 3} OR score fp32 [B][h][w] in [0, 1]
 * (the other pointer NULL); low_rgb / high_rgb 0xRRGGBB; scaler in [0, 1].  out fp32 [B][3][H][W] = k / 255 with, per image,
 *   lo, hi = min / max of the image, d = float32(max(double(hi) - double(lo), 1e-5)), p = (uint8)(((v - lo) / d) * 255);
 *   colour c: levels 2: high_c * g + low_c * (1 - g) in integers (exactly low or high for g in {0, 1}); levels 3 (s = float(g) / 2)
 *   and scores (s): (uint8)(float(high_c) * s + float(low_c) * (1 - s));
 *   k = (uint8)(float(p) + scaler * float(int(c) - int(p)))      [PIL's Image.blend]
 * The cell size is H / h: DVQ_ESHAPE unless h divides H, w divides W and H / h == W / w.
 * dvq_grain_lines: in place on x fp32 [B][3][H][W]: -1 on the top row and left column of every cell, for grain >= 1 on the row and
 * column at cell / 2, for grain == 2 on those at cell / 4 and cell - cell / 4 (draw_dual_grain_256res / draw_triple_grain_256res).
 * dvq_image_grid_u8: x fp32 [N][C][H][W], C in {1, 3} -> out uint8 [GH][GW][3] (a one-channel input is repeated), torchvision's
 * make_grid(nrow, padding, normalize=True, pad_value=0) followed by (uint8)(g * 255): optional clamp to [-1, 1], lo / hi over the WHOLE
 * tensor, d as above, g = (v - lo) / d.  Image k sits at row (k / xmaps) * (H + padding) + padding, column (k % xmaps) * (W + padding)
 * + padding, xmaps = min(nrow, N); padding and empty cells are 0; N == 1 gives the image itself, unpadded.  dvq_image_grid_shape
 * reports GH, GW; out_bytes < GH * GW * 3: DVQ_EWORKSPACE. */
size_t dvq_imagelog_workspace_bytes(int64_t segments);
int dvq_grain_overlay(const float* x, const int64_t* grain, const float* score, int levels, int64_t B, int64_t H, int64_t W, int64_t h,
                      int64_t w, uint32_t low_rgb, uint32_t high_rgb, float scaler, float* out, void* ws, size_t ws_bytes,
                      dvq_stream_t stream);
int dvq_grain_lines(float* x, const int64_t* grain, int levels, int64_t B, int64_t H, int64_t W, int64_t h, int64_t w,
                    dvq_stream_t stream);
int dvq_image_grid_shape(int64_t N, int64_t H, int64_t W, int64_t nrow, int64_t padding, int64_t* grid_h, int64_t* grid_w);
int dvq_image_grid_u8(const float* x, int64_t N, int64_t C, int64_t H, int64_t W, int64_t nrow, int64_t padding, int clamp, uint8_t* out,
                      size_t out_bytes, void* ws, size_t ws_bytes, dvq_stream_t stream);

/* Lossless token codec (csrc/codec.hip, docs/design/27-token-codec.md): rANS driven by the DQ-Transformer's next-token distributions.
 * The frequency table of a logits row [V <= DVQ_TOKEN_RULE_MAXV] of `dtype` (row pitch ldl) under `rule` (dvq_token_rule above, the
 * sampler's) is
 *   A = the columns the rule leaves to a live row and whose logit is finite (a finished row: {pad_code}), n = |A|, M = 65536;
 *   n == 1: f = M on that column;  n == 0: f = 0 everywhere;
 *   n >= 2: e_c = expf(x_c - max_A x), S = sum_A e_c in fp32 (lane l of 64 adds columns l, l + 64, ... in ascending order, then a fixed
 *           xor tree), f_c = 1 + floor(e_c / S * (M - n)) on A, 0 elsewhere, and M - sum f is added to the lowest-index arg-max of A.
 * The coder is rANS: 64-bit state, lower bound 2^31, 32-bit words, 16-bit frequencies, one state and one word stream per row.
 * err uint32 [B] is sticky (bits are only ever set): 1 = a target with f = 0 (or outside [0, V)), 2 = a read past the end of a stream
 * (it yields a zero word), 4 = a live row with an empty allowed set, 8 = internal (no column under the state).
 * dvq_codec_tables: table uint32 [B][V] = f.  For tests and inspection.
 * dvq_codec_record: records[row * rec_ld + step] = cum | f << 16 of target[row] (int64 [B]), or 0 when the step codes nothing (finished
 *   row, n == 1, or an error); token int64 [B] = the target for a live row (pad_code when it lies outside [0, V)), pad_code for a finished one.
 * dvq_codec_encode: records uint32 [B][rec_ld], the first min(counts[row], T) steps of a row are coded (counts int64 [B] or NULL: T), last
 *   to first; row b's words end at words + (b + 1) * cap (uint32 [B][cap], cap >= T + 2), nwords int64 [B] = how many: the stream is
 *   words[(b + 1) * cap - nwords[b] ...], its first two words the final state (low half first).  bits fp64 [B][3] or NULL: sum of
 *   16 - log2 f over the coded steps with kinds[step] = 0, 1, 2 (uint8 [T]; NULL: all 0; >= 3: not counted), in a fixed order.
 * dvq_codec_decode_step: state int64 [B][4] = {rANS state, cursor, index of the row's first word in `words`, words in its stream}
 *   (the caller starts with state = word 0 | word 1 << 32, cursor = 2); token int64 [B] = the column c with cum_c <= state mod M <
 *   cum_c + f_c (pad_code for a finished row, the one allowed column when n == 1); the state advances and refills at most one word
 *   from words[base + cursor] iff cursor < count and base + cursor < total_words -- otherwise a zero word and error bit 2. */
int dvq_codec_tables(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, const dvq_token_rule* rule, uint32_t* table,
                     dvq_stream_t stream);
int dvq_codec_record(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, const dvq_token_rule* rule, const int64_t* target,
                     uint32_t* records, int64_t rec_ld, int64_t step, int64_t* token, uint32_t* err, dvq_stream_t stream);
int dvq_codec_encode(const uint32_t* records, int64_t B, int64_t T, int64_t rec_ld, const int64_t* counts, const uint8_t* kinds,
                     uint32_t* words, int64_t cap, int64_t* nwords, double* bits, dvq_stream_t stream);
int dvq_codec_decode_step(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, const dvq_token_rule* rule, int64_t* state,
                          const uint32_t* words, int64_t total_words, int64_t* token, uint32_t* err, dvq_stream_t stream);

/* ---- sample-set metrics on feature vectors (csrc/sampleset.hip, docs/design/32-sample-set-metrics.md; no reference kernel: its
 * samplers stop at an .npz for an external tool) -----------------------------------------------------------------------------------
 * dvq_feat_moments: x fp32 [N][ld], the first D columns are used (columns D .. ld are never read); shift fp32 [D].  With
 *   y = fl32(x - shift):  sum fp64 [D] += sum_n y,  gram fp64 [D][D] += sum_n y y^T on the UPPER triangle (row <= column; the lower
 *   triangle is never touched: the caller mirrors it),  n int64 [1] += N.  The caller zeroes the three once and streams a set through
 *   in batches.  Every product of two fp32 values is formed exactly in fp64 and added in fp64, one owner per output walking the rows in
 *   order (plain fp64 FMAs): no atomics, the same batches give the same bits.  D in [1, 4096], N >= 1 (else DVQ_ESHAPE).
 * dvq_pair_scan: a fp32 [Na][lda], b fp32 [Nb][ldb], first D columns used (the rest never read).  With
 *   d2(i, j) = max(fl32(fl32(|a_i|^2 + |b_j|^2) - 2 a_i.b_j), 0): the norms summed in fp64 from exact squares and rounded once to fp32,
 *   the inner product fp32 fmaf chains on the fp32 matrix instruction (one per block of 64 columns, per 8 columns in the order 0, 4,
 *   1, 5, 2, 6, 3, 7; the block sums added in order -- blocked summation, a quarter of one long chain's error at D = 1024).  The form
 *   is accurate for CENTRED features only (error ~ 1e-7 (|a|^2 + |b|^2)): the caller subtracts a common mean first.  Per row i of a:
 *   kth2 fp32 [Na][k] = the k smallest d2(i, j), ascending, +inf where fewer than k candidates exist;  idx int64 [Na][k] = their j
 *   (equal distances: the lower j first), -1 at the padding;  count int64 [Na] = #{j : d2(i, j) <= rad2_b[j]} on the same d2 values
 *   (rad2_b fp32 [Nb]; NULL: count is not touched and may be NULL).  exclude_diag = 1 skips the pair j == i (a set against itself).
 *   k in [1, 16] and exclude_diag in {0, 1} (else DVQ_EINVAL); Na, Nb, D >= 1, Nb < 2^31, pitches >= D (else DVQ_ESHAPE).
 *   ws: dvq_pair_scan_workspace_bytes(Na, Nb, k) bytes, 8-byte aligned (per-split candidate lists when a has too few rows to fill the
 *   chip; 0 when b is not split, ws may then be NULL; 0 for bad arguments too; smaller: DVQ_EWORKSPACE, nothing is launched).  No
 *   Na x Nb array exists anywhere.  One owner per output and no float atomics: two launches give the same bits, and a row's result
 *   depends on that row of a and on b only -- not on the other rows of a, their number, or the split.
 *   Non-finite inputs: a pair whose d2 comes out NaN or +inf is neither selected nor counted (a row of a holding a NaN reports +inf / -1
 *   / 0 throughout); every idx written is -1 or in [0, Nb). */
int dvq_feat_moments(const float* x, int64_t N, int64_t D, int64_t ld, const float* shift, double* sum, double* gram, int64_t* n,
                     dvq_stream_t stream);
size_t dvq_pair_scan_workspace_bytes(int64_t Na, int64_t Nb, int k);
int dvq_pair_scan(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t Na, int64_t Nb, int64_t D, const float* rad2_b, int k,
                  int exclude_diag, float* kth2, int64_t* idx, int64_t* count, void* ws, size_t ws_bytes, dvq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DVQ_HIP_H */
