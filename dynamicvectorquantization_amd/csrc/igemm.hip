// Implicit-GEMM convolution + batched GEMM on MFMA for gfx950 (bf16 32x32x16 and exact-fp32 32x32x2).
//
// Replaces the torch.nn.Conv2d call sites of the DQ-VAE (modules/diffusionmodules/model.py:38-192 --
// ResnetBlock 3x3, Upsample nearest+3x3, Downsample pad+3x3/s2, AttnBlock 1x1 q/k/v/proj and the
// q.k / p.v batched matmuls -- plus quant_conv/post_quant_conv, dqvae_dual_entropy.py:93-94) and
// their autograd backward (dgrad = transposed gather, wgrad = pixel-dimension reduction).
//
// Two kernels share one LDS tile format and one MFMA inner loop:
//   NT  C[m][n]  = sum_k A[m][k] * B[n][k]      A rows are gathered on the fly (im2col never exists)
//   TN  C[i][j] += sum_m A[m][i] * B[m][j]      both operands are transposed 8x8 (4x4 fp32) in registers
//                                               on their way to LDS; split over m with fp32 atomics
//
// Map of the files:
//   igemm.h       host-side contract: NtParams / TnParams, MODE_*, launch_nt<T>, launch_tn<T>, launch_nt_skinny
//   igemm_dev.h   device pieces the three .hip files use: tile constants, swizzles, MFMA stage loops, fp32x3 split (split8_bf16), zero page
//   igemm_nt.hip  every NT kernel with its epilogues, predicates and launchers; launch_nt
//   igemm_tn.hip  every TN kernel with the deterministic fold, predicates and launchers; launch_tn
//   igemm.hip     this file, the front end: descriptor checks, params builders, the fp32x3 launch-level schemes (plane kernels, the scratch
//                 rule, the routes) and the extern "C" entry points that pick between them and the kernels of the two files above
#include "igemm.h"
#include "igemm_dev.h"

using namespace igemm;

namespace {

int conv_check(const dvq_conv_desc* d, const char* who) {
    dvq_note_kernel("");          // first statement of every conv entry point: no stale family from an earlier call
    DVQ_REQUIRE(d != nullptr, DVQ_EINVAL, "%s: null descriptor", who);
    DVQ_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->OH > 0 && d->OW > 0 && d->Cout > 0 && d->KH > 0 &&
                    d->KW > 0 && d->stride > 0 && d->pad_t >= 0 && d->pad_l >= 0,
                DVQ_ESHAPE, "%s: non-positive dimension", who);
    DVQ_REQUIRE(d->N * d->OH * d->OW < (1ll << 31) && d->N * d->H * d->W < (1ll << 31), DVQ_ESHAPE,
                "%s: more than 2^31 pixels", who);
    DVQ_REQUIRE(d->upsample == 0 || d->upsample == 1, DVQ_EINVAL, "%s: upsample must be 0 or 1 (2: dvq_conv2d_fwd / _dgrad only)", who);
    DVQ_REQUIRE(!d->upsample || (d->H % 2 == 0 && d->W % 2 == 0), DVQ_ESHAPE, "%s: upsample needs even H, W", who);
    DVQ_REQUIRE(d->dtype == DVQ_F32 || d->dtype == DVQ_BF16, DVQ_EINVAL, "%s: bad dtype", who);
    // the implied bottom/right padding must keep every tap within one pad of the input
    DVQ_REQUIRE((d->OH - 1) * d->stride - d->pad_t + d->KH - 1 < d->H + d->KH && (d->OW - 1) * d->stride - d->pad_l + d->KW - 1 < d->W + d->KW,
                DVQ_ESHAPE, "%s: inconsistent output size", who);
    return DVQ_OK;
}

}  // namespace

// conv_halo.hip: LDS-resident-halo kernel for 3x3 / stride 1 / pad 1 bf16 convolutions (1 = handled, 0 = not eligible)
int dvq_conv3x3_halo_try(const void* x, const void* w, const float* bias, const void* residual, void* y, int64_t N,
                         int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flip, int up, const float* gn_ss,
                         double* out_stats, int out_groups, float act_slope, int res_mask, float mask_slope,
                         hipStream_t stream);

int dvq_conv3x3_halo_wgrad_try(const void* x, const void* dy, float* dw, float* db, int64_t N, int64_t H, int64_t W,
                               int64_t Cin, int64_t Cout, int64_t cin_real, int64_t cout_real, int c_oihw, int up,
                               const float* gn_ss, hipStream_t stream);
int dvq_conv3x3_halo_wgrad_planes_try(const void* x_planes, const void* dy_planes, float* dw, float* db, int64_t N, int64_t H, int64_t W,
                                      int64_t Cin, int64_t Cout, int64_t cin_real, int64_t cout_real, int c_oihw, int up, hipStream_t stream);

int dvq_conv3x3_thin_k_try(const void* x, const void* w, const float* bias, void* y, int64_t N, int64_t H, int64_t W, int64_t Cout,
                           int flip, float act_slope, hipStream_t stream);

int dvq_tconv4x4s2_thin_try(const void* dy, const void* wt, void* dx, int64_t N, int64_t OH, int64_t OW, int64_t Cout, int creal,
                            hipStream_t stream);

// conv_halo.hip: nearest x2 + 3x3 as four 2x2 sub-pixel convolutions on the low-resolution tensor (h, w); dgrad = 1: the input gradient
int dvq_conv3x3_halo_subpixel_try(const void* x, const void* wsub, const float* bias, void* y, int64_t N, int64_t h, int64_t w, int64_t Cin,
                                  int64_t Cout, int dgrad, double* out_stats, int out_groups, hipStream_t stream);

// A/B builds: -DDVQ_UPS_SUBPIXEL=0 (DVQ_BUILD_EXTRA_FLAGS) keeps every folded upsample on the 9-tap form
#ifndef DVQ_UPS_SUBPIXEL
#define DVQ_UPS_SUBPIXEL 1
#endif

static float act_slope_of(int act) { return act == DVQ_ACT_RELU ? 0.f : act == DVQ_ACT_LRELU ? 0.2f : 1.f; }

int dvq_conv3x3_halo_out32_try(const void* x, const void* w, const float* bias, const float* residual, float* y, int64_t N,
                               int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flip, int up, float act_slope, int res_mask,
                               float mask_slope, hipStream_t stream);

// -------------------------------------------------------------------------------------------------
// fp32x3 at LAUNCH level (round 5): the three products of the split scheme -- lo.hi + hi.lo + hi.hi, see split8_bf16 -- on the bf16
// kernels, from bf16 PLANES of the fp32 operands (hi = RNE(x), lo = RNE(x - hi)) that an HBM-bound pass writes once per operand into
// caller-provided scratch, instead of the fp32 kernels that split at every fragment read.  dvq_conv2d_fwd / _dgrad / _wgrad take these
// routes when the caller hands them scratch (x3_route); dvq_conv2d_scratch_bytes is the size rule (x3_scratch_need).
//
// Forward / input gradient of the 3 x 3 / stride 1 / pad 1 convolutions on the HALO kernel (conv_x3_halo).  The three products are laid
// side by side on the channel axis of bf16 operands -- x' = [x_hi | x_lo | x_hi] and, per tap, w' = [w_hi | w_hi | w_lo], 3 Cin channels --
// so ONE launch of the bf16 halo kernel forms x_hi.w_hi + x_lo.w_hi + x_hi.w_lo in its fp32 accumulators, and its fp32-output
// instantiation (conv_halo.hip, OUT32) stores them unrounded, after the fp32 residual / gate / activation.  Same products, same
// accumulation type as the in-kernel split of igemm_nt_glds_kernel<float, S3>, on a kernel that stages every activation once for all 9
// taps (the fp32 kernel: 200 - 250 TFLOP/s nominal, bound by its 2-us stages, section 3 of DESIGN.md).  Costs: one pass writes x' (4 B
// read + 6 B written per element), the weights are re-laid per call (Cout x 9 x Cin elements).
//
// Weight gradients (conv_wgrad_x3).  A weight gradient is accumulated in fp32 whatever the operand type (atomics or partials + fold into
// the fp32 gradient), so the three products can be three launches of the bf16 weight-gradient kernels (halo / patch / transpose-read:
// 600 - 1200 TFLOP/s) instead of one launch of the register-staged fp32 kernel (140 - 190 TFLOP/s nominal, and 9 passes over the
// activations for a 3 x 3 kernel).  Planes cost 4 B read, 4 B written per element; channels are padded from the fp32 layout's multiple
// of 4 to the bf16 kernels' multiple of 8 on the way.
// -------------------------------------------------------------------------------------------------
namespace {

// Both plane kernels: one thread per 8 channels, two 16-B loads, split8_bf16, 16-B stores.
// split_concat3_kernel: planes side by side on the channel axis.  MODE 0 (activations): [hi | lo | hi]; MODE 1 (weights, rows = Cout x 9):
// [hi | hi | lo].  c % 8 == 0.
template <int MODE>
__global__ __launch_bounds__(256) void split_concat3_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int64_t rows, int c) {
    const int cpr = c >> 3;
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cpr;
        const int c0 = (int)(i - r * cpr) << 3;
        const float* src = x + r * c + c0;
        bf16x8 h, l;
        split8_bf16(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), h, l);
        bf16_t* dst = out + r * 3 * c + c0;
        *reinterpret_cast<bf16x8*>(dst) = h;
        *reinterpret_cast<bf16x8*>(dst + c) = MODE == 0 ? l : h;
        *reinterpret_cast<bf16x8*>(dst + 2 * c) = MODE == 0 ? h : l;
    }
}

// separate planes of `cout` channels each; channels >= cin are zero
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo,
                                                           int64_t rows, int cin, int cout) {
    const int cpr = cout >> 3;                          // 8-channel chunks per output row
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cpr;
        const int c0 = (int)(i - r * cpr) << 3;
        const float* src = x + r * cin + c0;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
        if (c0 < cin) a = *reinterpret_cast<const f32x4*>(src);            // cin % 4 == 0
        if (c0 + 4 < cin) b = *reinterpret_cast<const f32x4*>(src + 4);
        bf16x8 h, l;
        split8_bf16(a, b, h, l);
        *reinterpret_cast<bf16x8*>(hi + r * cout + c0) = h;
        *reinterpret_cast<bf16x8*>(lo + r * cout + c0) = l;
    }
}

int split_concat3(const float* x, void* out, int64_t rows, int64_t c, int mode, hipStream_t s) {
    const int64_t total = rows * (c / 8);
    int64_t blocks = cdiv64(total, 256);
    if (blocks > 256 * 64) blocks = 256 * 64;
    if (mode == 0) split_concat3_kernel<0><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(x, (bf16_t*)out, rows, (int)c);
    else split_concat3_kernel<1><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(x, (bf16_t*)out, rows, (int)c);
    DVQ_CHECK_LAUNCH("split_concat3");
    return DVQ_OK;
}

inline int64_t pad8(int64_t c) { return (c + 7) & ~(int64_t)7; }
inline int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// shapes conv_x3_halo takes.  cs: channels of the streamed operand (x: Cin / dy: Cout), co: channels produced
bool x3_halo_shape_ok(const dvq_conv_desc* d, int64_t cs, int64_t co) {
    return d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->OH == d->H && d->OW == d->W && d->H % 8 == 0 &&
           d->W % 32 == 0 && cs % 64 == 0 && co >= 4 && co % 4 == 0 && d->N * d->H * d->W * (3 * cs > co ? 3 * cs : co) < (1ll << 31) &&
           co * 27 * cs < (1ll << 31) && d->H * d->W * co * 4 < (1ll << 31);
}

// dvq_conv2d_scratch_bytes: what the launch-level route of `pass` wants for this descriptor, 0 when there is no such route
int64_t x3_scratch_need(const dvq_conv_desc* d, int pass) {
    if (d->dtype != DVQ_F32 || d->impl != DVQ_IMPL_AUTO || !dvq_fp32_split()) return 0;
    const int64_t xrows = d->N * (d->H >> d->upsample) * (d->W >> d->upsample), yrows = d->N * d->OH * d->OW;
    if (pass == DVQ_PASS_WGRAD)
        return 4 * (xrows * pad8(d->Cin) + yrows * pad8(d->Cout)) + 1024;       // two bf16 planes per operand, 256-B aligned starts
    const bool dgrad = pass == DVQ_PASS_DGRAD;
    const int64_t cs = dgrad ? d->Cout : d->Cin, co = dgrad ? d->Cin : d->Cout;
    if (!x3_halo_shape_ok(d, cs, co)) return 0;
    return up256((dgrad ? d->N * d->H * d->W : xrows) * 3 * cs * 2) + up256(co * 9 * 3 * cs * 2);
}

// 1: this call takes the launch-level route of `pass` (it wants scratch and got some); 0: it does not; DVQ_EWORKSPACE: bad scratch
int x3_route(const dvq_conv_desc* d, int pass, const void* scratch, int64_t scratch_bytes, const char* who) {
    const int64_t need = x3_scratch_need(d, pass);
    if (need == 0 || scratch == nullptr) return 0;
    DVQ_REQUIRE(scratch_bytes >= need && ((uintptr_t)scratch & 15) == 0, DVQ_EWORKSPACE,
                "%s: scratch smaller than dvq_conv2d_scratch_bytes or not 16-B aligned", who);
    return 1;
}

}  // namespace

static bool halo_eligible(const dvq_conv_desc* d) {
    return d->dtype == DVQ_BF16 && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 &&
           d->OH == d->H && d->OW == d->W && (d->impl == DVQ_IMPL_AUTO || d->impl == DVQ_IMPL_HALO);
}

// Shapes whose folded nearest-x2 upsample runs as four 2x2 sub-pixel convolutions (conv_halo.hip, SUB): bf16 halo shapes with the tile
// grid on the LOW resolution and whole 64-channel chunks on both sides
static bool subpixel_eligible(const dvq_conv_desc* d) {
    const int64_t h = d->H / 2, w = d->W / 2;
    return DVQ_UPS_SUBPIXEL && d->upsample && halo_eligible(d) && d->H % 2 == 0 && d->W % 2 == 0 && h % 8 == 0 && w % 32 == 0 &&
           d->Cin % 64 == 0 && d->Cout % 64 == 0 && d->N * d->H * d->W * (d->Cin > d->Cout ? d->Cin : d->Cout) < (1ll << 30) &&
           d->Cout * 16 * d->Cin < (1ll << 30);
}

// dvq_conv2d_fwd / dvq_conv2d_dgrad: upsample == 2 is upsample == 1 with the sub-pixel pack behind the 3x3 pack of the weight argument
// (dvq_pack_weight, bit 9 of dtype); every other entry, and everything behind these two, sees 0 / 1
static int conv_check_up2(dvq_conv_desc* dd, const char* who) {
    const bool sub = dd->upsample == 2;
    if (sub) dd->upsample = 1;
    if (int e = conv_check(dd, who)) return e;
    DVQ_REQUIRE(!sub || subpixel_eligible(dd), DVQ_ESHAPE, "%s: upsample == 2 needs a shape accepted by dvq_conv3x3_subpixel_ok", who);
    return sub ? 1 : DVQ_OK;
}

// NtParams of a convolution pass.  MODE_FWD: A = x streams d->Cin channels, C = y is the output map; MODE_TCONV (input gradient): A = dy
// streams d->Cout channels, C is the gradient at the LOGICAL input resolution (a folded upsample is summed down by the caller).
static NtParams conv_nt_params(const dvq_conv_desc* d, int mode, const void* A, const void* B, void* C) {
    const bool fwd = mode == MODE_FWD;
    const int64_t cs = fwd ? d->Cin : d->Cout, co = fwd ? d->Cout : d->Cin;      // channels streamed / produced
    NtParams p{};
    p.A = A; p.B = B; p.C = C;
    p.mode = mode;
    p.M = (int)(fwd ? d->N * d->OH * d->OW : d->N * d->H * d->W); p.Ncols = (int)co; p.Ktot = (int)(d->KH * d->KW * cs);
    p.lda = cs; p.ldb = p.Ktot; p.ldc = co;
    if (fwd) {
        p.SH = (int)(d->H >> d->upsample); p.SW = (int)(d->W >> d->upsample);
        p.LH = (int)d->H; p.LW = (int)d->W; p.DH = (int)d->OH; p.DW = (int)d->OW;
        p.up = d->upsample;
    } else {
        p.SH = (int)d->OH; p.SW = (int)d->OW; p.LH = (int)d->OH; p.LW = (int)d->OW;
        p.DH = (int)d->H; p.DW = (int)d->W;
    }
    p.KW = d->KW; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.alpha = 1.f; p.act_slope = 1.f;
    return p;
}

// TnParams of a convolution's weight gradient; rows / columns beyond the real channel counts are padding
static TnParams conv_tn_params(const dvq_conv_desc* d, const void* x, const void* dy, int64_t cin_real, int64_t cout_real, float* grad,
                               float* dbias, int ohwi) {
    TnParams p{};
    p.A = dy; p.B = x; p.C = grad; p.colsumA = dbias;
    p.conv = 1;
    p.Mred = (int)(d->N * d->OH * d->OW); p.I = (int)cout_real; p.J = (int)d->Cin;
    p.lda = d->Cout; p.ldb = d->Cin; p.ldc = (int64_t)d->KH * d->KW * d->Cin;
    p.taps = d->KH * d->KW;
    p.SH = (int)(d->H >> d->upsample); p.SW = (int)(d->W >> d->upsample);
    p.LH = (int)d->H; p.LW = (int)d->W; p.DH = (int)d->OH; p.DW = (int)d->OW;
    p.KW = d->KW; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l; p.up = d->upsample;
    p.c_oihw = ohwi ? 0 : 1; p.Jc = (int)cin_real;
    if (ohwi) p.ldc = (int64_t)d->KH * d->KW * cin_real;
    return p;
}

static NtParams gemm_nt_params(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                               int64_t sA, int64_t sB, int64_t sC, float alpha, const float* bias, int bias_mode) {
    NtParams p{};
    p.A = A; p.B = B; p.C = C; p.R = nullptr; p.bias = bias;
    p.mode = MODE_GEMM;
    p.M = (int)M; p.Ncols = (int)N; p.Ktot = (int)K;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.stride = 1; p.KW = 1;
    p.alpha = alpha; p.bias_mode = bias_mode;
    p.act_slope = 1.f;
    p.sA = sA; p.sB = sB; p.sC = sC;
    return p;
}

static TnParams gemm_tn_params(const void* A, const void* B, float* C, float* colsum, int64_t Mred, int64_t I, int64_t J, int64_t lda,
                               int64_t ldb, int64_t ldc, int64_t sA, int64_t sB, int64_t sC) {
    TnParams p{};
    p.A = A; p.B = B; p.C = C; p.colsumA = colsum;
    p.conv = 0;
    p.Mred = (int)Mred; p.I = (int)I; p.J = (int)J;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.taps = 1; p.KW = 1; p.stride = 1;
    p.Jc = p.J;
    p.sA = sA; p.sB = sB; p.sC = sC;
    return p;
}

int dvq_sumpool2x2(const void* in, int dtype, int64_t N, int64_t h, int64_t w, int64_t C, void* out, dvq_stream_t stream);

// fp32x3 forward (dgrad = 0: a = x, wgt = w) / input gradient (dgrad = 1: a = dy, wgt = wt, res = the mask, out at the logical input
// resolution) on the halo kernel: concatenated planes into scratch, one OUT32 launch
static int conv_x3_halo(const dvq_conv_desc* d, int dgrad, const void* a, const void* wgt, const float* bias, const void* res, void* out,
                        float act_slope, int res_mask, float mask_slope, void* scratch, hipStream_t stream) {
    const int64_t cs = dgrad ? d->Cout : d->Cin, co = dgrad ? d->Cin : d->Cout;
    const int64_t rows = dgrad ? d->N * d->H * d->W : d->N * (d->H >> d->upsample) * (d->W >> d->upsample);
    char* as = (char*)scratch;
    char* ws = as + up256(rows * 3 * cs * 2);
    if (int e = split_concat3((const float*)a, as, rows, cs, 0, stream)) return e;
    if (int e = split_concat3((const float*)wgt, ws, co * 9, cs, 1, stream)) return e;
    const int rc = dvq_conv3x3_halo_out32_try(as, ws, bias, (const float*)res, (float*)out, d->N, d->H, d->W, 3 * cs, co, dgrad,
                                              dgrad ? 0 : d->upsample, act_slope, res_mask, mask_slope, stream);
    if (rc < 0) return rc;
    DVQ_REQUIRE(rc == 1, DVQ_ESHAPE, "fp32x3 convolution: the halo kernel refused the shape");
    dvq_note_kernel("conv_x3_halo");              // the route's label, over the halo kernel's own note
    return DVQ_OK;
}

// the weight gradient behind dvq_conv2d_wgrad's argument checks
static int conv_wgrad(const dvq_conv_desc* d, const void* x, const void* dy, int64_t cin_real, int64_t cout_real, float* grad, float* dbias,
                      int ohwi, const float* gn_scale_shift, hipStream_t stream) {
    if (halo_eligible(d)) {
        const int rc = dvq_conv3x3_halo_wgrad_try(x, dy, grad, dbias, d->N, d->H, d->W, d->Cin, d->Cout, cin_real,
                                                  cout_real, ohwi ? 0 : 1, d->upsample, gn_scale_shift, stream);
        if (rc != 0) return rc < 0 ? rc : DVQ_OK;
    }
    DVQ_REQUIRE(gn_scale_shift == nullptr, DVQ_ESHAPE, "dvq_conv2d_wgrad: fused GroupNorm needs a shape accepted by dvq_conv3x3_fused_ok");
    DVQ_REQUIRE(d->impl != DVQ_IMPL_HALO, DVQ_ESHAPE, "dvq_conv2d_wgrad: shape not eligible for the halo kernel");
    const TnParams p = conv_tn_params(d, x, dy, cin_real, cout_real, grad, dbias, ohwi);
    if (d->dtype == DVQ_F32) return launch_tn<float>(p, 1, d->impl, stream);
    return launch_tn<bf16_t>(p, 1, d->impl, stream);
}

// fp32x3 weight gradient: bf16 planes of both operands into scratch, then the bf16 weight gradient over them
static int conv_wgrad_x3(const dvq_conv_desc* d, const void* x, const void* dy, int64_t cin_real, int64_t cout_real, float* grad,
                         float* dbias, int ohwi, void* scratch, hipStream_t stream) {
    const int64_t xrows = d->N * (d->H >> d->upsample) * (d->W >> d->upsample), yrows = d->N * d->OH * d->OW;
    const int64_t c8 = pad8(d->Cin), o8 = pad8(d->Cout);
    char* xh = (char*)scratch;
    char* xl = xh + up256(xrows * c8 * 2);
    char* yh = xl + up256(xrows * c8 * 2);
    char* yl = yh + up256(yrows * o8 * 2);
    if (int e = dvq_split_bf16_planes((const float*)x, xh, xl, xrows, d->Cin, c8, stream)) return e;
    if (int e = dvq_split_bf16_planes((const float*)dy, yh, yl, yrows, d->Cout, o8, stream)) return e;
    dvq_conv_desc b = *d;
    b.dtype = DVQ_BF16;
    b.Cin = c8;
    b.Cout = o8;
    // 3 x 3 / stride 1 / pad 1 on the halo kernel: ONE launch over "3 N images" -- image n of plane triple (x_lo, dy_hi), (x_hi, dy_lo),
    // (x_hi, dy_hi) -- instead of three launches with three folds of the partials (the planes of an operand are contiguous: eligible
    // shapes have plane sizes that are multiples of 256 bytes).  Shapes the halo kernel does not take: three launches
    int rc = 0;
    if (halo_eligible(&b) && xl == xh + xrows * c8 * 2 && yl == yh + yrows * o8 * 2)
        rc = dvq_conv3x3_halo_wgrad_planes_try(xh, yh, grad, dbias, d->N, d->H, d->W, c8, o8, cin_real, cout_real, ohwi ? 0 : 1, d->upsample,
                                               stream);
    if (rc < 0) return rc;
    if (rc == 0) {
        // small terms first; the bias gradient (column sums of dy) is the sum over BOTH dy planes, taken on the two launches that read x_hi
        if (int e = conv_wgrad(&b, xl, yh, cin_real, cout_real, grad, nullptr, ohwi, nullptr, stream)) return e;
        if (int e = conv_wgrad(&b, xh, yl, cin_real, cout_real, grad, dbias, ohwi, nullptr, stream)) return e;
        if (int e = conv_wgrad(&b, xh, yh, cin_real, cout_real, grad, dbias, ohwi, nullptr, stream)) return e;
    }
    dvq_note_kernel("conv_wgrad_x3_planes");      // the route's label, over the note of the kernel that ran last
    return DVQ_OK;
}

// =================================================================================================
extern "C" {

int dvq_conv3x3_fused_ok(const dvq_conv_desc* d) {
    // shapes on which the halo kernels (and therefore the fused GroupNorm prologue / statistics epilogue) run
    return d != nullptr && halo_eligible(d) && d->H % 8 == 0 && d->W % 32 == 0 && d->Cin % 64 == 0 && d->Cout % 8 == 0 &&
           d->N * d->H * d->W * (d->Cin > d->Cout ? d->Cin : d->Cout) < (1ll << 31);
}

int dvq_conv3x3_subpixel_ok(const dvq_conv_desc* d) {
    if (d == nullptr || d->upsample == 0) return 0;
    dvq_conv_desc dd = *d;
    dd.upsample = 1;
    return subpixel_eligible(&dd);
}

int dvq_conv2d_fwd(const dvq_conv_desc* d_in, const void* x, const void* w, const float* bias, const void* residual, void* y,
                   const float* gn_scale_shift, double* out_stats, int out_groups, int act, void* scratch, int64_t scratch_bytes,
                   dvq_stream_t stream) {
    dvq_note_kernel("");
    DVQ_REQUIRE(d_in != nullptr, DVQ_EINVAL, "dvq_conv2d_fwd: null descriptor");
    dvq_conv_desc dd = *d_in;
    const dvq_conv_desc* d = &dd;
    const int sub = conv_check_up2(&dd, "dvq_conv2d_fwd");
    if (sub < 0) return sub;
    DVQ_REQUIRE(act == DVQ_ACT_NONE || act == DVQ_ACT_RELU || act == DVQ_ACT_LRELU, DVQ_EINVAL, "dvq_conv2d_fwd: bad act");
    DVQ_REQUIRE(act == DVQ_ACT_NONE || (residual == nullptr && gn_scale_shift == nullptr && out_stats == nullptr), DVQ_EINVAL,
                "dvq_conv2d_fwd: activation together with residual, gn_scale_shift or out_stats");
    DVQ_REQUIRE(x && w && y, DVQ_EINVAL, "dvq_conv2d_fwd: null pointer");
    const int x3 = gn_scale_shift || out_stats ? 0 : x3_route(d, DVQ_PASS_FWD, scratch, scratch_bytes, "dvq_conv2d_fwd");
    if (x3 < 0) return x3;
    if (x3) return conv_x3_halo(d, 0, x, w, bias, residual, y, act_slope_of(act), 0, 0.f, scratch, (hipStream_t)stream);
    if (halo_eligible(d) && d->impl == DVQ_IMPL_AUTO && d->Cin == 8 && !d->upsample && residual == nullptr && gn_scale_shift == nullptr &&
        out_stats == nullptr) {          // image heads: 8 (padded) input channels
        const int rc = dvq_conv3x3_thin_k_try(x, w, bias, y, d->N, d->H, d->W, d->Cout, 0, act_slope_of(act), (hipStream_t)stream);
        if (rc != 0) return rc < 0 ? rc : DVQ_OK;
    }
    if (sub && residual == nullptr && gn_scale_shift == nullptr && act == DVQ_ACT_NONE) {
        const bf16_t* wsub = (const bf16_t*)w + d->Cout * 9 * d->Cin;
        const int rc = dvq_conv3x3_halo_subpixel_try(x, wsub, bias, y, d->N, d->H / 2, d->W / 2, d->Cin, d->Cout, 0, out_stats, out_groups,
                                                     (hipStream_t)stream);
        if (rc != 0) return rc < 0 ? rc : DVQ_OK;
    }
    if (halo_eligible(d)) {
        const int rc = dvq_conv3x3_halo_try(x, w, bias, residual, y, d->N, d->H, d->W, d->Cin, d->Cout, 0, d->upsample,
                                            gn_scale_shift, out_stats, out_groups, act_slope_of(act), 0, 0.f,
                                            (hipStream_t)stream);
        if (rc != 0) return rc < 0 ? rc : DVQ_OK;
    }
    DVQ_REQUIRE(gn_scale_shift == nullptr && out_stats == nullptr, DVQ_ESHAPE,
                "dvq_conv2d_fwd: fused GroupNorm needs a shape accepted by dvq_conv3x3_fused_ok");
    DVQ_REQUIRE(d->impl != DVQ_IMPL_HALO, DVQ_ESHAPE, "dvq_conv2d_fwd: shape not eligible for the halo kernel");
    NtParams p = conv_nt_params(d, MODE_FWD, x, w, y);
    p.R = residual; p.bias = bias; p.bias_mode = bias ? 1 : 0;
    p.act_slope = act_slope_of(act);
    if (d->dtype == DVQ_F32) return launch_nt<float>(p, 1, d->impl, (hipStream_t)stream);
    return launch_nt<bf16_t>(p, 1, d->impl, (hipStream_t)stream);
}

int dvq_conv2d_dgrad(const dvq_conv_desc* d_in, const void* dy, const void* wt, void* dx, void* ws, const void* mask, int mask_act,
                     void* scratch, int64_t scratch_bytes, dvq_stream_t stream) {
    dvq_note_kernel("");
    DVQ_REQUIRE(d_in != nullptr, DVQ_EINVAL, "dvq_conv2d_dgrad: null descriptor");
    dvq_conv_desc dd = *d_in;
    const dvq_conv_desc* d = &dd;
    const int sub = conv_check_up2(&dd, "dvq_conv2d_dgrad");
    if (sub < 0) return sub;
    DVQ_REQUIRE(mask == nullptr || ((mask_act == DVQ_ACT_RELU || mask_act == DVQ_ACT_LRELU) && !d->upsample), DVQ_EINVAL,
                "dvq_conv2d_dgrad: mask needs act in {relu, lrelu} and no folded upsample");
    DVQ_REQUIRE(dy && wt && dx && (!d->upsample || ws || sub), DVQ_EINVAL, "dvq_conv2d_dgrad: null pointer");
    const int x3 = x3_route(d, DVQ_PASS_DGRAD, scratch, scratch_bytes, "dvq_conv2d_dgrad");
    if (x3 < 0) return x3;
    if (x3) {
        if (int e = conv_x3_halo(d, 1, dy, wt, nullptr, mask, d->upsample ? ws : dx, 1.f, mask != nullptr, act_slope_of(mask_act), scratch,
                                 (hipStream_t)stream))
            return e;
        return d->upsample ? dvq_sumpool2x2(ws, d->dtype, d->N, d->H / 2, d->W / 2, d->Cin, dx, stream) : DVQ_OK;
    }
    if (sub) {
        // the low-resolution gradient straight from one fp32 accumulation: ws is not touched, no 2x2 sum pass
        const bf16_t* wsub = (const bf16_t*)wt + d->Cin * 9 * d->Cout;
        const int rc = dvq_conv3x3_halo_subpixel_try(dy, wsub, nullptr, dx, d->N, d->H / 2, d->W / 2, d->Cin, d->Cout, 1, nullptr, 0,
                                                     (hipStream_t)stream);
        if (rc < 0) return rc;
        DVQ_REQUIRE(rc == 1, DVQ_ESHAPE, "dvq_conv2d_dgrad: the halo kernel refused the sub-pixel form");
        return DVQ_OK;
    }
    if (d->dtype == DVQ_BF16 && d->impl == DVQ_IMPL_AUTO && d->KH == 4 && d->KW == 4 && d->stride == 2 && d->pad_t == 1 && d->pad_l == 1 &&
        d->Cin == 8 && !d->upsample && mask == nullptr && d->H == 2 * d->OH && d->W == 2 * d->OW) {
        // input gradient of the PatchGAN's first conv (3 image channels): thin transposed conv
        const int rc = dvq_tconv4x4s2_thin_try(dy, wt, dx, d->N, d->OH, d->OW, d->Cout, 4, (hipStream_t)stream);
        if (rc != 0) return rc < 0 ? rc : DVQ_OK;
    }
    if (halo_eligible(d) && d->impl == DVQ_IMPL_AUTO && d->Cout == 8 && !d->upsample && mask == nullptr) {
        // dgrad of the 3-channel output conv: 8 gradient channels in, Cin out, taps reversed
        const int rc = dvq_conv3x3_thin_k_try(dy, wt, nullptr, dx, d->N, d->H, d->W, d->Cin, 1, 1.f, (hipStream_t)stream);
        if (rc != 0) return rc < 0 ? rc : DVQ_OK;
    }
    if (halo_eligible(d)) {      // dgrad of a 3x3/s1/p1 conv = the same conv over dy with the taps reversed
        // with a folded nearest-x2 upsample the gradient is formed at the upsampled resolution (ws), then 2x2-summed
        const int rc = dvq_conv3x3_halo_try(dy, wt, nullptr, mask, d->upsample ? ws : dx, d->N, d->H, d->W, d->Cout, d->Cin, 1,
                                            0, nullptr, nullptr, 0, 1.f, mask != nullptr, act_slope_of(mask_act),
                                            (hipStream_t)stream);
        if (rc < 0) return rc;
        if (rc == 1) return d->upsample ? dvq_sumpool2x2(ws, d->dtype, d->N, d->H / 2, d->W / 2, d->Cin, dx, stream) : DVQ_OK;
    }
    DVQ_REQUIRE(d->impl != DVQ_IMPL_HALO, DVQ_ESHAPE, "dvq_conv2d_dgrad: shape not eligible for the halo kernel");
    NtParams p = conv_nt_params(d, MODE_TCONV, dy, wt, d->upsample ? ws : dx);
    p.R = mask; p.res_mask = mask != nullptr; p.mask_slope = act_slope_of(mask_act);
    int rc = d->dtype == DVQ_F32 ? launch_nt<float>(p, 1, d->impl, (hipStream_t)stream)
                                 : launch_nt<bf16_t>(p, 1, d->impl, (hipStream_t)stream);
    if (rc) return rc;
    if (d->upsample) return dvq_sumpool2x2(ws, d->dtype, d->N, d->H / 2, d->W / 2, d->Cin, dx, stream);
    return DVQ_OK;
}

int dvq_conv2d_wgrad(const dvq_conv_desc* d, const void* x, const void* dy, int64_t cin_real, int64_t cout_real, float* grad,
                     float* dbias, int ohwi, const float* gn_scale_shift, void* scratch, int64_t scratch_bytes, dvq_stream_t stream) {
    if (int e = conv_check(d, "dvq_conv2d_wgrad")) return e;
    DVQ_REQUIRE(x && dy && grad && cin_real > 0 && cin_real <= d->Cin && cout_real > 0 && cout_real <= d->Cout,
                DVQ_EINVAL, "dvq_conv2d_wgrad: bad arguments");
    const int x3 = gn_scale_shift ? 0 : x3_route(d, DVQ_PASS_WGRAD, scratch, scratch_bytes, "dvq_conv2d_wgrad");
    if (x3 < 0) return x3;
    if (x3) return conv_wgrad_x3(d, x, dy, cin_real, cout_real, grad, dbias, ohwi, scratch, (hipStream_t)stream);
    return conv_wgrad(d, x, dy, cin_real, cout_real, grad, dbias, ohwi, gn_scale_shift, (hipStream_t)stream);
}

int64_t dvq_conv2d_scratch_bytes(const dvq_conv_desc* d, int pass) {
    if (d == nullptr || pass < DVQ_PASS_FWD || pass > DVQ_PASS_WGRAD || d->upsample < 0 || d->upsample > 1) return 0;
    return x3_scratch_need(d, pass);
}

int dvq_split_bf16_planes(const float* x, void* hi, void* lo, int64_t rows, int64_t cin, int64_t cout, dvq_stream_t stream) {
    DVQ_REQUIRE(x && hi && lo, DVQ_EINVAL, "dvq_split_bf16_planes: null pointer");
    DVQ_REQUIRE(rows > 0 && cin > 0 && cin % 4 == 0 && cout % 8 == 0 && cout >= cin && cout < (1 << 20), DVQ_ESHAPE,
                "dvq_split_bf16_planes: needs cin %% 4 == 0, cout %% 8 == 0, cout >= cin");
    const int64_t total = rows * (cout / 8);
    int64_t blocks = cdiv64(total, 256);
    if (blocks > 256 * 64) blocks = 256 * 64;
    split_planes_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(x, (bf16_t*)hi, (bf16_t*)lo, rows, (int)cin, (int)cout);
    DVQ_CHECK_LAUNCH("split_planes");
    return DVQ_OK;
}

int dvq_gemm_nt(const void* A, const void* B, void* C, int dtype, int64_t M, int64_t N, int64_t K, int64_t lda,
                int64_t ldb, int64_t ldc, int64_t batch, int64_t sA, int64_t sB, int64_t sC, float alpha,
                const float* bias, int bias_mode, int impl, dvq_stream_t stream) {
    dvq_note_kernel("");
    DVQ_REQUIRE(A && B && C, DVQ_EINVAL, "dvq_gemm_nt: null pointer");
    DVQ_REQUIRE(M > 0 && N > 0 && K > 0 && batch > 0 && batch <= 65535 && M < (1ll << 31) && N < (1ll << 31), DVQ_ESHAPE,
                "dvq_gemm_nt: bad shape");
    DVQ_REQUIRE(bias_mode == 0 || bias != nullptr, DVQ_EINVAL, "dvq_gemm_nt: bias_mode without bias");
    const NtParams p = gemm_nt_params(A, B, C, M, N, K, lda, ldb, ldc, sA, sB, sC, alpha, bias, bias_mode);
    if (dtype == DVQ_BF16 && impl == DVQ_IMPL_AUTO && batch == 1 && bias_mode != 2 && M <= 32 && N >= 64 && K >= 64 && K % 8 == 0 &&
        lda % 8 == 0 && ldb % 8 == 0)
        return launch_nt_skinny(p, (hipStream_t)stream);      // single-token Linear layers of the sampler: weight-streaming kernel
    if (dtype == DVQ_F32) return launch_nt<float>(p, batch, impl, (hipStream_t)stream);
    if (dtype == DVQ_BF16) return launch_nt<bf16_t>(p, batch, impl, (hipStream_t)stream);
    dvq_set_error("dvq_gemm_nt: bad dtype");
    return DVQ_EINVAL;
}

int dvq_gemm_tn(const void* A, const void* B, float* C, float* colsum, int dtype, int64_t Mred, int64_t I, int64_t J, int64_t lda,
                int64_t ldb, int64_t ldc, int64_t batch, int64_t sA, int64_t sB, int64_t sC, int impl, dvq_stream_t stream) {
    dvq_note_kernel("");
    DVQ_REQUIRE(A && B && C, DVQ_EINVAL, "dvq_gemm_tn: null pointer");
    DVQ_REQUIRE(Mred > 0 && I > 0 && J > 0 && batch > 0 && batch <= 65535 && Mred < (1ll << 31), DVQ_ESHAPE,
                "dvq_gemm_tn: bad shape");
    DVQ_REQUIRE(colsum == nullptr || batch == 1, DVQ_EINVAL, "dvq_gemm_tn: colsum needs batch 1");
    const TnParams p = gemm_tn_params(A, B, C, colsum, Mred, I, J, lda, ldb, ldc, sA, sB, sC);
    if (dtype == DVQ_F32) return launch_tn<float>(p, batch, impl, (hipStream_t)stream);
    if (dtype == DVQ_BF16) return launch_tn<bf16_t>(p, batch, impl, (hipStream_t)stream);
    dvq_set_error("dvq_gemm_tn: bad dtype");
    return DVQ_EINVAL;
}

}  // extern "C"
