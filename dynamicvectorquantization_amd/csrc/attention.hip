// Fused causal multi-head self-attention of the stage-2 transformer (bf16), forward and backward.  The kernels of this file are causal
// only and serve head size 64; causal head size 128 and the DQ-VAE's full attention (one head of 256) run on attention2.hip.  The C ABI
// entry points and the geometry check of both kernel sets are at the end of this file:
//   CausalSelfAttention.forward   modules/dynamic_modules/stackgpt.py:41-69
//       att = softmax(mask(q k^T / sqrt(hs)));  att = attn_drop(att);  y = att v
// The unfused path (per-head GEMMs + softmax + dropout kernels, stackgpt.py of this package) moves the [B, nh, T, T] score
// tensor through HBM five times per layer and direction; here it never leaves registers (flash-attention recurrence).
//
// MFMA 32x32x16 bf16 operand/accumulator layout (A[i][k], B[k][n], C[i][n]; lane = 64 threads, half = lane >> 5):
//   A: lane -> i = lane & 31, holds k = 8 * half + j (j = 0..7)      B: lane -> n = lane & 31, holds k = 8 * half + j
//   C: lane -> n = lane & 31, register r -> i = (r & 3) + 8 * (r >> 2) + 4 * half
// Every kernel keeps the SOFTMAX ROW INDEX OR THE CONTRACTED INDEX on the accumulator's register axis so that no
// shuffle / LDS transpose is ever needed between the two GEMMs of a tile:
//   forward, dQ:   S^T[key][query] = K Q^T   (lane = query: the row statistics are per-lane scalars; registers = keys,
//                  which is the contraction index of the second GEMM  O^T[ch][query] = V^T[ch][key] P^T[key][query])
//   dK / dV:       S[query][key] = Q K^T     (lane = key; registers = queries = contraction index of
//                  dV^T[ch][key] = dO^T[ch][query] P[query][key],  dK^T[ch][key] = Q^T[ch][query] dS[query][key])
// The second GEMM's k index is PERMUTED to the accumulator's register order (k = 8 * half + j  <->  register 8 * s + j,
// i.e. row (j & 3) + 8 * (2 s + (j >> 2)) + 4 * half): the B operand is then the accumulator itself (converted to bf16) and
// the A operand -- read from a channel-major (transposed) copy of V / K / Q / dO -- is two 8-byte loads of 4 consecutive
// rows.
// One wave per 32-row tile; the 4 waves of a workgroup own 4 neighbouring tiles of the same (batch, head) and walk the
// other sequence axis together: each 32-row operand tile is fetched from global memory ONCE per workgroup into registers
// (issued one tile ahead), published through double-buffered LDS (one barrier per tile) and read by all four waves as MFMA
// fragments (padded rows: conflict-free ds_read_b128 / ds_read_b64).  Waves beyond their causal range idle for <= 3 tiles.
#include <type_traits>

#include "attn_common.h"

namespace {

// LDS tile geometry: row-major tiles [32 rows][HS channels] (K, V, Q, dO) and channel-major tiles [HS channels][32 rows]
// (V^T, K^T, Q^T, dO^T); row strides padded by 16 bytes
template <int HS>
struct Geo {
    static constexpr int RROW = HS * 2 + 16;          // bytes per row of a row-major tile
    static constexpr int CROW = 64 + 16;              // bytes per channel of a channel-major tile
    static constexpr int RTILE = 32 * RROW;
    static constexpr int CTILE = HS * CROW;
    static constexpr int NCH = HS / 64;               // 16-byte chunks per thread and tile (256 threads)
};

// global -> registers: rows r0 .. r0+31 of a row-major [.., C] matrix (head slice of HS channels); rows >= T read as zero
template <int HS>
__device__ __forceinline__ void gload_rows(const bf16_t* base, int64_t rowbase, int r0, int T, int C, int tid, uint4 (&reg)[HS / 64]) {
#pragma unroll
    for (int i = 0; i < HS / 64; ++i) {
        const int id = tid + 256 * i, row = id / (HS / 8), cc = id % (HS / 8);
        reg[i] = r0 + row < T ? *reinterpret_cast<const uint4*>(base + (rowbase + r0 + row) * C + cc * 8) : make_uint4(0, 0, 0, 0);
    }
}
template <int HS>
__device__ __forceinline__ void swrite_rows(char* tile, int tid, const uint4 (&reg)[HS / 64]) {
#pragma unroll
    for (int i = 0; i < HS / 64; ++i) {
        const int id = tid + 256 * i, row = id / (HS / 8), cc = id % (HS / 8);
        *reinterpret_cast<uint4*>(tile + row * Geo<HS>::RROW + cc * 16) = reg[i];
    }
}
// global -> registers: columns r0 .. r0+31 of a channel-major [HS channels][T] slice; columns >= T read as zero (T % 8 == 0)
template <int HS>
__device__ __forceinline__ void gload_cols(const bf16_t* base, int r0, int T, int tid, uint4 (&reg)[HS / 64]) {
#pragma unroll
    for (int i = 0; i < HS / 64; ++i) {
        const int id = tid + 256 * i, ch = id >> 2, kc = id & 3;
        reg[i] = r0 + kc * 8 < T ? *reinterpret_cast<const uint4*>(base + (int64_t)ch * T + r0 + kc * 8) : make_uint4(0, 0, 0, 0);
    }
}
template <int HS>
__device__ __forceinline__ void swrite_cols(char* tile, int tid, const uint4 (&reg)[HS / 64]) {
#pragma unroll
    for (int i = 0; i < HS / 64; ++i) {
        const int id = tid + 256 * i, ch = id >> 2, kc = id & 3;
        *reinterpret_cast<uint4*>(tile + ch * Geo<HS>::CROW + kc * 16) = reg[i];
    }
}

// MFMA fragments from LDS tiles.  Row-major tile: lane -> row l31, channels 16 st + 8 half .. +7
template <int HS>
__device__ __forceinline__ bf16x8 frag_r(const char* tile, int l31, int half, int st) {
    return *reinterpret_cast<const bf16x8*>(tile + l31 * Geo<HS>::RROW + (16 * st + 8 * half) * 2);
}
// channel-major tile, permuted-k A operand: lane -> channel 32 mt + l31, rows 16 s2 + 4 half + {0..3, 8..11}
template <int HS>
__device__ __forceinline__ bf16x8 frag_c(const char* tile, int l31, int half, int mt, int s2) {
    const char* q = tile + (32 * mt + l31) * Geo<HS>::CROW + (16 * s2 + 4 * half) * 2;
    Frag f;
    f.h[0] = *reinterpret_cast<const uint2*>(q);
    f.h[1] = *reinterpret_cast<const uint2*>(q + 16);
    return f.v;
}

// ------------------------------------------------------------------------------------------------------------------
// forward: one wave per 32 queries; the workgroup walks the key tiles 0 .. (its last query tile)
// ------------------------------------------------------------------------------------------------------------------
// (two workgroups per CU: without the explicit bound the compiler spreads into AGPRs and settles for one wave per SIMD)
template <int HS>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnArgsCm p) {
    using G = Geo<HS>;
    constexpr int NS = HS / 16, NM = HS / 32, STAGE = G::RTILE + G::CTILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int T = p.T, C = p.nh * HS;
    const int bh = blockIdx.y, b = bh / p.nh, h = bh - b * p.nh;
    const int nqt = (T + 31) / 32;
    const int qt_max = nqt - 1 - blockIdx.x * 4;                 // late (long) query tiles first; wave 0 owns the last one
    const int qt = qt_max - wave;
    const bool active = qt >= 0;
    const int q0 = qt * 32, qrow = q0 + l31;
    const bool qok = active && qrow < T;
    const int64_t rowbase = (int64_t)b * T;
    bf16x8 qf[NS];
    {
        const bf16_t* qp = p.q + (rowbase + qrow) * C + h * HS + 8 * half;
#pragma unroll
        for (int s = 0; s < NS; ++s) qf[s] = ldfrag(qp + 16 * s, qok);
    }
    f32x16 oacc[NM];
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) oacc[mt] = zero16();
    float m_run = -INFINITY, l_run = 0.f;                       // running max (log2 domain) and sum
    const float c2 = p.scale * LOG2E;
    const unsigned idx_row = (unsigned)(((int64_t)bh * T + qrow) * T);
    const bf16_t* kbase = p.k + h * HS;
    const bf16_t* vtbase = p.vt + ((int64_t)b * C + h * HS) * T;
    uint4 rk[G::NCH], rv[G::NCH];
    gload_rows<HS>(kbase, rowbase, 0, T, C, tid, rk);
    gload_cols<HS>(vtbase, 0, T, tid, rv);
    swrite_rows<HS>(smem, tid, rk);
    swrite_cols<HS>(smem + G::RTILE, tid, rv);
    __syncthreads();
    for (int kt = 0; kt <= qt_max; ++kt) {
        const char* kl = smem + (kt & 1) * STAGE;
        const char* vl = kl + G::RTILE;
        const bool more = kt < qt_max;
        if (more) {
            gload_rows<HS>(kbase, rowbase, 32 * (kt + 1), T, C, tid, rk);
            gload_cols<HS>(vtbase, 32 * (kt + 1), T, tid, rv);
        }
        if (active && kt <= qt) {
            const int k0 = kt * 32;
            f32x16 s = zero16();
#pragma unroll
            for (int st = 0; st < NS; ++st) s = MFMA(frag_r<HS>(kl, l31, half, st), qf[st], s);
            float mx = m_run;
            if (kt == qt) {                                       // diagonal tile: causal mask (also hides keys >= T)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + crow(r, half);
                    s[r] = (key <= qrow && key < T) ? s[r] * c2 : -INFINITY;
                    mx = fmaxf(mx, s[r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] *= c2;
                    mx = fmaxf(mx, s[r]);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mref = mx == -INFINITY ? 0.f : mx;       // rows without any valid key (padding rows only)
            const float alpha = __builtin_amdgcn_exp2f(m_run - mref);
            float rs = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = __builtin_amdgcn_exp2f(s[r] - mref);
                rs += s[r];
            }
            rs += __shfl_xor(rs, 32, 64);
            l_run = l_run * alpha + rs;
            m_run = mx;
            if (!__all(alpha == 1.f)) {                          // the running maximum settles after a few tiles
#pragma unroll
                for (int mt = 0; mt < NM; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[mt][r] *= alpha;
            }
            if (p.thr != 0) {
                unsigned long long mine = 0;                     // lane r keeps the ballot of register r
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned idx = idx_row + (unsigned)(k0 + crow(r, half));
                    const bool keep = dvq_hash32(idx * p.rm + p.ra) >= p.thr;
                    if (p.mask != nullptr) {
                        const unsigned long long m = __ballot(keep);
                        mine = lane == r ? m : mine;
                    }
                    s[r] = keep ? s[r] * p.inv_keep : 0.f;
                }
                if (p.mask != nullptr && lane < 16) p.mask[drop_tile(bh, nqt, qt, kt) + lane] = mine;
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 pf = pack8(s, s2);
#pragma unroll
                for (int mt = 0; mt < NM; ++mt) oacc[mt] = MFMA(frag_c<HS>(vl, l31, half, mt, s2), pf, oacc[mt]);
            }
        }
        if (more) {
            char* nl = smem + ((kt + 1) & 1) * STAGE;
            swrite_rows<HS>(nl, tid, rk);
            swrite_cols<HS>(nl + G::RTILE, tid, rv);
        }
        __syncthreads();
    }
    if (qok) {
        store_ct<NM>(p.out + (rowbase + qrow) * C + h * HS, oacc, half, 1.f / l_run);
        if (half == 0) p.lse[(int64_t)bh * T + qrow] = (m_run + __builtin_amdgcn_logf(l_run)) * (1.f / LOG2E);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// backward, dQ: one wave per 32 queries (same walk as the forward); LDS stage = K, V (row-major) and K^T tiles
// ------------------------------------------------------------------------------------------------------------------
template <int HS, bool MASKED = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(AttnArgsCm p) {
    using G = Geo<HS>;
    constexpr int NS = HS / 16, NM = HS / 32, STAGE = 2 * G::RTILE + G::CTILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int T = p.T, C = p.nh * HS;
    const int bh = blockIdx.y, b = bh / p.nh, h = bh - b * p.nh;
    const int nqt = (T + 31) / 32;
    const int qt_max = nqt - 1 - blockIdx.x * 4;
    const int qt = qt_max - wave;
    const bool active = qt >= 0;
    const int q0 = qt * 32, qrow = q0 + l31;
    const bool qok = active && qrow < T;
    const int64_t rowbase = (int64_t)b * T;
    bf16x8 qf[NS], dof[NS];
    {
        const bf16_t* qp = p.q + (rowbase + qrow) * C + h * HS + 8 * half;
        const bf16_t* dop = p.dout + (rowbase + qrow) * C + h * HS + 8 * half;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            qf[s] = ldfrag(qp + 16 * s, qok);
            dof[s] = ldfrag(dop + 16 * s, qok);
        }
    }
    const float lq = qok ? p.lse[(int64_t)bh * T + qrow] * LOG2E : 0.f;
    // dsum[query] = sum_ch dO * O: taken here from the dO fragments this wave holds anyway (+ the matching O fragments) and left in
    // p.dsum for the dK kernel, which is launched after this one (a separate one-thread-per-row pass over dO and O was 38 us per layer)
    float dq_ = 0.f;
    {
        const bf16_t* op = p.o + (rowbase + qrow) * C + h * HS + 8 * half;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            Frag fo, fd;
            fo.v = ldfrag(op + 16 * s, qok);
            fd.v = dof[s];
            const unsigned* a = &fo.u.x;
            const unsigned* b2 = &fd.u.x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dq_ = fmaf(__uint_as_float(a[j] << 16), __uint_as_float(b2[j] << 16), dq_);
                dq_ = fmaf(__uint_as_float(a[j] & 0xffff0000u), __uint_as_float(b2[j] & 0xffff0000u), dq_);
            }
        }
        dq_ += __shfl_xor(dq_, 32, 64);
        if (qok && half == 0) p.dsum[(int64_t)bh * T + qrow] = dq_;
    }
    f32x16 acc[NM];                                              // dQ^T [ch][query]
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) acc[mt] = zero16();
    const float c2 = p.scale * LOG2E;
    const unsigned idx_row = (unsigned)(((int64_t)bh * T + qrow) * T);
    const bf16_t* kbase = p.k + h * HS;
    const bf16_t* vbase = p.v + h * HS;
    const bf16_t* ktbase = p.kt + ((int64_t)b * C + h * HS) * T;
    uint4 rk[G::NCH], rv[G::NCH], rt[G::NCH];
    gload_rows<HS>(kbase, rowbase, 0, T, C, tid, rk);
    gload_rows<HS>(vbase, rowbase, 0, T, C, tid, rv);
    gload_cols<HS>(ktbase, 0, T, tid, rt);
    swrite_rows<HS>(smem, tid, rk);
    swrite_rows<HS>(smem + G::RTILE, tid, rv);
    swrite_cols<HS>(smem + 2 * G::RTILE, tid, rt);
    __syncthreads();
    for (int kt = 0; kt <= qt_max; ++kt) {
        const char* kl = smem + (kt & 1) * STAGE;
        const char* vl = kl + G::RTILE;
        const char* tl = kl + 2 * G::RTILE;
        const bool more = kt < qt_max;
        if (more) {
            gload_rows<HS>(kbase, rowbase, 32 * (kt + 1), T, C, tid, rk);
            gload_rows<HS>(vbase, rowbase, 32 * (kt + 1), T, C, tid, rv);
            gload_cols<HS>(ktbase, 32 * (kt + 1), T, tid, rt);
        }
        if (active && kt <= qt) {
            const int k0 = kt * 32;
            unsigned long long mk[16];                           // the tile's 16 select masks: scalar loads, issued ahead of the first GEMMs
            if constexpr (MASKED) {
                const unsigned long long* mw = p.mask + drop_tile(bh, nqt, __builtin_amdgcn_readfirstlane(qt), kt);
#pragma unroll
                for (int r = 0; r < 16; ++r) mk[r] = mw[r];
            }
            f32x16 s = zero16(), dp = zero16();
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                s = MFMA(frag_r<HS>(kl, l31, half, st), qf[st], s);
                dp = MFMA(frag_r<HS>(vl, l31, half, st), dof[st], dp);
            }
            auto elementwise = [&](auto diag_c) {
                constexpr bool DIAG = decltype(diag_c)::value, MASK = MASKED;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + crow(r, half);
                    float pr = __builtin_amdgcn_exp2f(s[r] * c2 - lq);
                    if constexpr (DIAG) pr = (key <= qrow && key < T) ? pr : 0.f;
                    float g = dp[r];
                    if constexpr (MASK) {
                        g = __builtin_amdgcn_inverse_ballot_w64(mk[r]) ? g * p.inv_keep : 0.f;
                    } else {
                        if (p.thr != 0) g = dvq_hash32((idx_row + (unsigned)key) * p.rm + p.ra) >= p.thr ? g * p.inv_keep : 0.f;
                    }
                    s[r] = pr * (g - dq_);                        // d loss / d (scaled score)
                }
            };
            if (kt == qt) elementwise(std::true_type{});
            else elementwise(std::false_type{});
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 df = pack8(s, s2);
#pragma unroll
                for (int mt = 0; mt < NM; ++mt) acc[mt] = MFMA(frag_c<HS>(tl, l31, half, mt, s2), df, acc[mt]);
            }
        }
        if (more) {
            char* nl = smem + ((kt + 1) & 1) * STAGE;
            swrite_rows<HS>(nl, tid, rk);
            swrite_rows<HS>(nl + G::RTILE, tid, rv);
            swrite_cols<HS>(nl + 2 * G::RTILE, tid, rt);
        }
        __syncthreads();
    }
    if (qok) store_ct<NM>(p.dq + (rowbase + qrow) * C + h * HS, acc, half, p.scale);
}

// ------------------------------------------------------------------------------------------------------------------
// backward, dK and dV: one wave per 32 keys; the workgroup walks the query tiles from its first key tile to the end;
// LDS stage = Q, dO (row-major) and Q^T, dO^T tiles
// ------------------------------------------------------------------------------------------------------------------
// MODE 0: dK and dV together (the one launch head size 64 makes); 1: dV only; 2: dK only.
template <int HS, int MODE = 0, bool MASKED = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(AttnArgsCm p) {
    constexpr bool DO_DV = MODE != 2, DO_DK = MODE != 1;
    using G = Geo<HS>;
    constexpr int NS = HS / 16, NM = HS / 32, STAGE = 2 * G::RTILE + 2 * G::CTILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int T = p.T, C = p.nh * HS;
    const int bh = blockIdx.y, b = bh / p.nh, h = bh - b * p.nh;
    const int nt = (T + 31) / 32;
    const int kt_min = blockIdx.x * 4;                            // early (long) key tiles first
    const int kt = kt_min + wave;
    const bool active = kt < nt;
    const int k0 = kt * 32, krow = k0 + l31;
    const bool kok = active && krow < T;
    const int64_t rowbase = (int64_t)b * T;
    bf16x8 kf[NS], vf[NS];
    {
        const bf16_t* kp = p.k + (rowbase + krow) * C + h * HS + 8 * half;
        const bf16_t* vp = p.v + (rowbase + krow) * C + h * HS + 8 * half;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            kf[s] = ldfrag(kp + 16 * s, kok);
            if constexpr (DO_DK) vf[s] = ldfrag(vp + 16 * s, kok);
        }
    }
    f32x16 dv[NM], dk[NM];                                        // dV^T, dK^T [ch][key]
#pragma unroll
    for (int mt = 0; mt < NM; ++mt) dv[mt] = dk[mt] = zero16();
    const float c2 = p.scale * LOG2E;
    const bf16_t* qbase = p.q + h * HS;
    const bf16_t* dobase = p.dout + h * HS;
    const bf16_t* qtbase = p.qt + ((int64_t)b * C + h * HS) * T;
    const bf16_t* dotbase = p.dot + ((int64_t)b * C + h * HS) * T;
    const float* lsep = p.lse + (int64_t)bh * T;
    const float* dsp = p.dsum + (int64_t)bh * T;
    uint4 rq[G::NCH], rd[G::NCH], rqt[G::NCH], rdt[G::NCH];
    gload_rows<HS>(qbase, rowbase, 32 * kt_min, T, C, tid, rq);
    if constexpr (DO_DK) gload_rows<HS>(dobase, rowbase, 32 * kt_min, T, C, tid, rd);
    if constexpr (DO_DK) gload_cols<HS>(qtbase, 32 * kt_min, T, tid, rqt);
    if constexpr (DO_DV) gload_cols<HS>(dotbase, 32 * kt_min, T, tid, rdt);
    swrite_rows<HS>(smem, tid, rq);
    if constexpr (DO_DK) swrite_rows<HS>(smem + G::RTILE, tid, rd);
    if constexpr (DO_DK) swrite_cols<HS>(smem + 2 * G::RTILE, tid, rqt);
    if constexpr (DO_DV) swrite_cols<HS>(smem + 2 * G::RTILE + G::CTILE, tid, rdt);
    __syncthreads();
    constexpr bool masked = MASKED;
    // keep bits of this lane's key over a tile's 32 queries (see drop_tile): one 4-byte load per tile, fetched one tile ahead
    const unsigned* mlane = reinterpret_cast<const unsigned*>(p.mask) + 2 * ((l31 & 3) + 4 * (l31 >> 3)) + ((l31 >> 2) & 1);
    auto mask_word = [&](int qt_) { return masked && active && qt_ >= kt ? mlane[2 * drop_tile(bh, nt, qt_, kt)] : 0u; };
    unsigned mnext = mask_word(kt_min);
    for (int qt = kt_min; qt < nt; ++qt) {
        const unsigned mword = mnext >> (4 * half);              // query 8 g + 4 half + i of the tile is bit 8 g + i
        if (qt + 1 < nt) mnext = mask_word(qt + 1);
        const char* ql = smem + ((qt - kt_min) & 1) * STAGE;
        const char* dl = ql + G::RTILE;
        const char* qtl = ql + 2 * G::RTILE;
        const char* dtl = qtl + G::CTILE;
        const bool more = qt + 1 < nt;
        if (more) {
            gload_rows<HS>(qbase, rowbase, 32 * (qt + 1), T, C, tid, rq);
            if constexpr (DO_DK) gload_rows<HS>(dobase, rowbase, 32 * (qt + 1), T, C, tid, rd);
            if constexpr (DO_DK) gload_cols<HS>(qtbase, 32 * (qt + 1), T, tid, rqt);
            if constexpr (DO_DV) gload_cols<HS>(dotbase, 32 * (qt + 1), T, tid, rdt);
        }
        if (active && qt >= kt) {
            const int q0 = qt * 32;
            f32x16 s = zero16(), dp = zero16();
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                s = MFMA(frag_r<HS>(ql, l31, half, st), kf[st], s);
                if constexpr (DO_DK) dp = MFMA(frag_r<HS>(dl, l31, half, st), vf[st], dp);
            }
            // element-wise pass and second GEMMs in two halves (registers 8 s2 .. 8 s2 + 7 = two groups of 4 consecutive
            // queries each): only 8 probabilities / 8 score gradients and 8 per-query statistics are live at a time
            const bool diag = qt == kt;
            const bool edge = diag || q0 + 32 > T;               // tiles that need per-element validity tests
            auto second = [&](auto edge_c) {
                constexpr bool EDGE = decltype(edge_c)::value, MASK = MASKED;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    Frag pf, df;
#pragma unroll
                    for (int gg = 0; gg < 2; ++gg) {
                        const int g = 2 * s2 + gg;
                        const int qq = q0 + 8 * g + 4 * half;
                        const bool ok = !EDGE || qq < T;              // T % 4 == 0: a group is entirely in or out
                        const float4 l4 = ok ? *reinterpret_cast<const float4*>(lsep + qq) : make_float4(0.f, 0.f, 0.f, 0.f);
                        const float4 d4 = ok ? *reinterpret_cast<const float4*>(dsp + qq) : make_float4(0.f, 0.f, 0.f, 0.f);
                        const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq_[4] = {d4.x, d4.y, d4.z, d4.w};
                        float pk[4], ds[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int r = 4 * g + i;
                            const int query = qq + i;
                            float pr = __builtin_amdgcn_exp2f(s[r] * c2 - lq[i] * LOG2E);
                            if constexpr (EDGE) pr = (ok && (!diag || krow <= query)) ? pr : 0.f;
                            float gr = dp[r];
                            pk[i] = pr;
                            if constexpr (MASK) {
                                const bool keep = (mword >> (8 * g + i)) & 1u;
                                gr = keep ? gr * p.inv_keep : 0.f;
                                pk[i] = keep ? pr * p.inv_keep : 0.f;
                            } else {
                                if (p.thr != 0) {
                                    const unsigned idx = (unsigned)(((int64_t)bh * T + query) * T) + (unsigned)krow;
                                    const bool keep = dvq_hash32(idx * p.rm + p.ra) >= p.thr;
                                    gr = keep ? gr * p.inv_keep : 0.f;
                                    pk[i] = keep ? pr * p.inv_keep : 0.f;
                                }
                            }
                            ds[i] = pr * (gr - dq_[i]);           // d loss / d (scaled score): dK;  pk: dropped-out probabilities: dV
                        }
                        const unsigned p0 = pack_bf16x2(pk[0], pk[1]), p1 = pack_bf16x2(pk[2], pk[3]);
                        const unsigned d0 = pack_bf16x2(ds[0], ds[1]), d1 = pack_bf16x2(ds[2], ds[3]);
                        if (gg == 0) {
                            pf.u.x = p0; pf.u.y = p1; df.u.x = d0; df.u.y = d1;
                        } else {
                            pf.u.z = p0; pf.u.w = p1; df.u.z = d0; df.u.w = d1;
                        }
                    }
#pragma unroll
                    for (int mt = 0; mt < NM; ++mt) {
                        if constexpr (DO_DV) dv[mt] = MFMA(frag_c<HS>(dtl, l31, half, mt, s2), pf.v, dv[mt]);
                        if constexpr (DO_DK) dk[mt] = MFMA(frag_c<HS>(qtl, l31, half, mt, s2), df.v, dk[mt]);
                    }
                }
            };
            if (edge) second(std::true_type{});
            else second(std::false_type{});
        }
        if (more) {
            char* nl = smem + ((qt + 1 - kt_min) & 1) * STAGE;
            swrite_rows<HS>(nl, tid, rq);
            if constexpr (DO_DK) swrite_rows<HS>(nl + G::RTILE, tid, rd);
            if constexpr (DO_DK) swrite_cols<HS>(nl + 2 * G::RTILE, tid, rqt);
            if constexpr (DO_DV) swrite_cols<HS>(nl + 2 * G::RTILE + G::CTILE, tid, rdt);
        }
        __syncthreads();
    }
    if (kok) {
        if constexpr (DO_DV) store_ct<NM>(p.dv + (rowbase + krow) * C + h * HS, dv, half, 1.f);
        if constexpr (DO_DK) store_ct<NM>(p.dk + (rowbase + krow) * C + h * HS, dk, half, p.scale);
    }
}

template <int HS>
int launch_fwd(const AttnArgsCm& p, dim3 grid, hipStream_t stream) {
    using G = Geo<HS>;
    const int lds = 2 * (G::RTILE + G::CTILE);
    dvq_ensure_dynamic_lds((const void*)attn_fwd_kernel<HS>, lds);
    attn_fwd_kernel<HS><<<grid, dim3(256), lds, stream>>>(p);
    return 0;
}

template <int HS, bool MASKED>
int launch_bwd_m(const AttnArgsCm& p, dim3 grid, hipStream_t stream) {
    using G = Geo<HS>;
    const int lds_kv = 2 * (2 * G::RTILE + 2 * G::CTILE), lds_q = 2 * (2 * G::RTILE + G::CTILE);
    dvq_ensure_dynamic_lds((const void*)attn_bwd_dq_kernel<HS, MASKED>, lds_q);
    attn_bwd_dq_kernel<HS, MASKED><<<grid, dim3(256), lds_q, stream>>>(p);        // first: it also produces dsum for the dK kernel
    dvq_ensure_dynamic_lds((const void*)attn_bwd_dkv_kernel<HS, 0, MASKED>, lds_kv);
    attn_bwd_dkv_kernel<HS, 0, MASKED><<<grid, dim3(256), lds_kv, stream>>>(p);
    return 0;
}
template <int HS>
int launch_bwd(const AttnArgsCm& p, dim3 grid, hipStream_t stream) {
    if (p.thr != 0 && p.mask != nullptr) return launch_bwd_m<HS, true>(p, grid, stream);
    return launch_bwd_m<HS, false>(p, grid, stream);
}

// geometry the fused kernels take, stated once: fill_params (every entry point) and the exported predicates dvq_attn_causal_ok /
// dvq_attn_full_ok ask it.  nullptr = accepted, else the refusal's format (one %s: the entry point).  ld: row pitch of q, k, v and
// their gradients.  Full attention (!causal) has no dropout path: attention2.hip launches nothing for it.
const char* attn_refusal(int dtype, int64_t B, int64_t T, int n_head, int head_dim, int64_t ld, float p_drop, int causal) {
    if (!(dtype == DVQ_BF16 && (causal ? head_dim == 64 || head_dim == 128 : head_dim == 256)))
        return "%s: bf16 with head size 64 or 128 (causal) / 256 (full attention) only (use the GEMM path otherwise)";
    if (!(causal || T % 32 == 0)) return "%s: full attention needs T %% 32 == 0";
    if (!(B > 0 && T > 0 && T % 8 == 0 && n_head > 0 && B * n_head <= 65535 && p_drop >= 0.f && p_drop < 1.f && (causal || p_drop == 0.f)))
        return "%s: bad geometry (T %% 8 == 0, B * n_head <= 65535)";
    if (!((double)B * n_head * (double)T * (double)T < 4294967296.0))
        return "%s: B * n_head * T * T must stay below 2^32 (dropout element index)";
    if (ld != (int64_t)n_head * head_dim && head_dim != 128)
        return "%s: a row pitch other than n_head * head_dim needs head size 128 (the kernels of attention2.hip)";
    if (!(ld >= (int64_t)n_head * head_dim && ld % 8 == 0 && (double)T * (double)ld * 2.0 < 4294967296.0))
        return "%s: bad pitch (at least n_head * head_dim, a multiple of 8, T * pitch * 2 below 2^32)";
    return nullptr;
}

int fill_params(AttnArgs& p, const char* who, int dtype, int64_t B, int64_t T, int n_head, int head_dim, int64_t ld, float scale, float p_drop,
                uint64_t seed, int causal = 1) {
    if (const char* why = attn_refusal(dtype, B, T, n_head, head_dim, ld, p_drop, causal)) {
        dvq_set_error(why, who);
        return DVQ_ESHAPE;
    }
    p.causal = causal;
    p.B = (int)B; p.T = (int)T; p.nh = n_head; p.ldq = (int)ld;
    p.scale = scale;
    p.inv_keep = 1.f / (1.f - p_drop);
    p.thr = (unsigned)((double)p_drop * 4294967296.0);
    dvq_dropout_seed(seed, &p.rm, &p.ra);
    return DVQ_OK;
}

int64_t dsum_bytes(int64_t B, int64_t T, int n_head) { return ((B * n_head * T * 4 + 255) / 256) * 256; }

}  // namespace

extern "C" {

int dvq_attn_causal_ok(int dtype, int64_t B, int64_t T, int n_head, int head_dim) {
    return attn_refusal(dtype, B, T, n_head, head_dim, (int64_t)n_head * head_dim, 0.f, 1) == nullptr;
}
int dvq_attn_full_ok(int dtype, int64_t B, int64_t T, int C) { return attn_refusal(dtype, B, T, 1, C, C, 0.f, 0) == nullptr; }

// head size 64: the channel-major copies (v^T forward; q^T, k^T, dO^T backward) and, behind them, dsum.  Head sizes 128 and 256
// (attention2.hip) read their operands in place: nothing forward, dsum alone backward.
int64_t dvq_attn_causal_scratch_bytes(int64_t B, int64_t T, int n_head, int head_dim, int backward) {
    const int64_t copy = head_dim == 64 ? B * T * n_head * head_dim * 2 : 0;
    return backward ? 3 * copy + dsum_bytes(B, T, n_head) : copy;
}

int64_t dvq_attn_causal_mask_bytes(int64_t B, int64_t T, int n_head) {
    const int64_t nt = (T + 31) / 32;
    return B * n_head * nt * nt * 16 * 8;
}

int dvq_attn_causal_fwd(const void* q, const void* k, const void* v, int64_t ldqkv, int dtype, int64_t B, int64_t T, int n_head,
                        int head_dim, float scale, float p_drop, uint64_t seed, void* out, float* lse, void* scratch, void* drop_mask,
                        dvq_stream_t stream) {
    DVQ_REQUIRE(q && k && v && out && lse, DVQ_EINVAL, "dvq_attn_causal_fwd: null pointer");
    AttnArgsCm p{};
    int rc = fill_params(p, "dvq_attn_causal_fwd", dtype, B, T, n_head, head_dim, ldqkv, scale, p_drop, seed);
    if (rc != DVQ_OK) return rc;
    DVQ_REQUIRE(scratch || dvq_attn_causal_scratch_bytes(B, T, n_head, head_dim, 0) == 0, DVQ_EINVAL, "dvq_attn_causal_fwd: null scratch");
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
    p.out = (bf16_t*)out; p.lse = lse;
    p.mask = (unsigned long long*)drop_mask;
    if (head_dim == 128) {
        dvq_attn2_fwd(p, (hipStream_t)stream);
        DVQ_CHECK_LAUNCH("attn_causal_fwd");
        return DVQ_OK;
    }
    p.vt = (const bf16_t*)scratch;
    rc = dvq_transpose(v, dtype, B, T, n_head * head_dim, scratch, stream);          // head size 64: v^T [B][C][T]
    if (rc != DVQ_OK) return rc;
    const int nqt = (int)((T + 31) / 32);
    launch_fwd<64>(p, dim3((unsigned)((nqt + 3) / 4), (unsigned)(B * n_head)), (hipStream_t)stream);
    DVQ_CHECK_LAUNCH("attn_causal_fwd");
    return DVQ_OK;
}

int dvq_attn_causal_bwd(const void* q, const void* k, const void* v, int64_t ldqkv, const void* out, const void* dout, const float* lse,
                        int dtype, int64_t B, int64_t T, int n_head, int head_dim, float scale, float p_drop, uint64_t seed, void* dq,
                        void* dk, void* dv, void* scratch, const void* drop_mask, dvq_stream_t stream) {
    DVQ_REQUIRE(q && k && v && out && dout && lse && dq && dk && dv && scratch, DVQ_EINVAL, "dvq_attn_causal_bwd: null pointer");
    AttnArgsCm p{};
    int rc = fill_params(p, "dvq_attn_causal_bwd", dtype, B, T, n_head, head_dim, ldqkv, scale, p_drop, seed);
    if (rc != DVQ_OK) return rc;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (const bf16_t*)out; p.dout = (const bf16_t*)dout;
    p.dq = (bf16_t*)dq; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv;
    p.lse = const_cast<float*>(lse);
    p.mask = (unsigned long long*)const_cast<void*>(drop_mask);
    if (head_dim == 128) {
        p.dsum = (float*)scratch;
        dvq_attn2_bwd(p, (hipStream_t)stream);
        DVQ_CHECK_LAUNCH("attn_causal_bwd");
        return DVQ_OK;
    }
    const int64_t C = n_head * head_dim, elems = B * T * C;                          // head size 64: q^T, k^T, dO^T [B][C][T], then dsum
    bf16_t* qt = (bf16_t*)scratch;
    bf16_t* kt = qt + elems;
    bf16_t* dot = kt + elems;
    p.qt = qt; p.kt = kt; p.dot = dot;
    p.dsum = reinterpret_cast<float*>(dot + elems);
    if ((rc = dvq_transpose(q, dtype, B, T, C, qt, stream)) != DVQ_OK) return rc;
    if ((rc = dvq_transpose(k, dtype, B, T, C, kt, stream)) != DVQ_OK) return rc;
    if ((rc = dvq_transpose(dout, dtype, B, T, C, dot, stream)) != DVQ_OK) return rc;
    const int nt = (int)((T + 31) / 32);
    launch_bwd<64>(p, dim3((unsigned)((nt + 3) / 4), (unsigned)(B * n_head)), (hipStream_t)stream);
    DVQ_CHECK_LAUNCH("attn_causal_bwd");
    return DVQ_OK;
}

/* ---- single-head FULL (non-causal) attention of the DQ-VAE's AttnBlock (modules/diffusionmodules/model.py:168-192): one head of
 * size C = 256 (attn_refusal takes no other), every query sees every key, no dropout; scores never reach HBM.  Scratch:
 * dvq_attn_causal_scratch_bytes with n_head = 1 (nothing forward, dsum backward). ---- */
int dvq_attn_full_fwd(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int C, float scale, void* out,
                      float* lse, void* /* scratch: none at this head size */, dvq_stream_t stream) {
    DVQ_REQUIRE(q && k && v && out && lse, DVQ_EINVAL, "dvq_attn_full_fwd: null pointer");
    AttnArgs p{};
    int rc = fill_params(p, "dvq_attn_full_fwd", dtype, B, T, 1, C, C, scale, 0.f, 0, 0);
    if (rc != DVQ_OK) return rc;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
    p.out = (bf16_t*)out; p.lse = lse;
    dvq_attn2_fwd(p, (hipStream_t)stream);
    DVQ_CHECK_LAUNCH("attn_full_fwd");
    return DVQ_OK;
}

int dvq_attn_full_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, int dtype,
                      int64_t B, int64_t T, int C, float scale, void* dq, void* dk, void* dv, void* scratch, dvq_stream_t stream) {
    DVQ_REQUIRE(q && k && v && out && dout && lse && dq && dk && dv && scratch, DVQ_EINVAL, "dvq_attn_full_bwd: null pointer");
    AttnArgs p{};
    int rc = fill_params(p, "dvq_attn_full_bwd", dtype, B, T, 1, C, C, scale, 0.f, 0, 0);
    if (rc != DVQ_OK) return rc;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (const bf16_t*)out; p.dout = (const bf16_t*)dout;
    p.dq = (bf16_t*)dq; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv;
    p.lse = const_cast<float*>(lse);
    p.dsum = (float*)scratch;
    dvq_attn2_bwd(p, (hipStream_t)stream);
    DVQ_CHECK_LAUNCH("attn_full_bwd");
    return DVQ_OK;
}

}  // extern "C"
