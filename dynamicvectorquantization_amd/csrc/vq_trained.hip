// Kernels of the gradient-trained codebook (MaskVectorQuantize, modules/vector_quantization/quantize_codebook_mask.py of the reference):
//   * dvq_vq_sample_argmax : argmax_k (s[n,k] / temp + gumbel(n,k)) without the [N,K] matrix, L2 or cosine scores
//   * dvq_vq_gumbel_noise  : the same noise as an explicit [N,K] matrix (tests / analysis)
//   * dvq_vq_codebook_grad : grad[k,:] += c * sum_{n: idx_n = k} m_n (e_k - x_n)
//   * dvq_vq_mask_ratio    : N / sum(mask) on the device (the loss' mask-ratio normalisation)
//   * dvq_vq_rownorm / dvq_vq_ortho_sumsq / dvq_vq_rownorm_bwd : the pieces of the orthogonality regulariser around the two GEMMs
//
// Scores.  For a fixed row the argmax over k of s[n,k] / temp + g does not change when a per-row constant is dropped, so
//   L2     : v[n,k] = (2 x_n.e_k - |e_k|^2) / temp + g(n,k)                       (the row's -|x_n|^2 / temp is dropped)
//   cosine : v[n,k] = x_n.ê_k / (max(|x_n|, 1e-12) temp) + g(n,k)                  (ê_k = e_k / max(|e_k|, 1e-12), prepared once)
// i.e. v = a_n * dot + b_k / temp with a per-row scale a_n and a per-code bias b_k.  temp == 0 means "no noise": v = a_n * dot + b_k.
// The dot product runs on bf16 MFMA with both operands split into two bf16 planes (x1.e1 + x1.e2 + x2.e1, fp32 accumulate: the
// scheme of vq.hip, ~3 * 2^-18 |x||e| per score); the noise arithmetic of a 32-code stage is VALU work issued behind the stage's MFMAs.
// The noisy search cannot prune and has no fp64 re-rank: a noise-perturbed score has no "exact" winner to defend.  The noiseless
// cosine search flags rows whose two best scores are within the evaluation bound and re-ranks them in fp64 (vq_cosine_rerank_kernel).
#include <type_traits>

#include "dvq_common.h"

namespace {

__host__ __device__ inline int64_t vqt_align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// prep buffer: bias [Kp] fp32 (-inf for padded codes) | plane e1 [Kp][D] bf16 | plane e2 [Kp][D] bf16 (zero rows for padded codes)
struct VqtPrep {
    float* bias;
    bf16_t* e1;
    bf16_t* e2;
    int64_t Kp;
};
__host__ __device__ inline VqtPrep vqt_prep_view(void* prep, int64_t K, int64_t D) {
    VqtPrep v;
    v.Kp = vqt_align_up(K, 32);
    char* p = (char*)prep;
    v.bias = (float*)p;
    const int64_t off = vqt_align_up(v.Kp * 4, 256);
    v.e1 = (bf16_t*)(p + off);
    v.e2 = (bf16_t*)(p + off + v.Kp * D * 2);
    return v;
}

// one wave per (padded) code
__global__ __launch_bounds__(256) void vqt_prepare_kernel(const float* __restrict__ cb, int64_t K, int64_t D, int cosine, void* prep) {
    VqtPrep pv = vqt_prep_view(prep, K, D);
    const int64_t k = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (k >= pv.Kp) return;
    double acc = 0.0;
    for (int64_t d = lane; d < D; d += 64) {
        const float e = k < K ? cb[k * D + d] : 0.0f;
        acc += (double)e * (double)e;
    }
    acc = wave_sum(acc);
    const float inv = cosine ? 1.0f / fmaxf((float)sqrt(acc), 1e-12f) : 1.0f;      // F.normalize: e / max(|e|, eps)
    for (int64_t d = lane; d < D; d += 64) {
        const float e = k < K ? cb[k * D + d] * inv : 0.0f;
        const bf16_t h = f32_to_bf16(e);
        pv.e1[k * D + d] = h;
        pv.e2[k * D + d] = f32_to_bf16(e - bf16_to_f32(h));
    }
    if (lane == 0) pv.bias[k] = k < K ? (cosine ? 0.0f : -(float)acc) : -__builtin_inff();
}

// ---- noise: counter-based, one value per (seed, draw counter, row, code) ------------------------------------------------------
__host__ __device__ __forceinline__ void vqt_key(uint64_t seed, uint64_t counter, unsigned& k0, unsigned& k1) {
    uint64_t key = seed * 0x9E3779B97F4A7C15ull + counter * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    key ^= key >> 29;
    key *= 0xBF58476D1CE4E5B9ull;
    key ^= key >> 32;
    k0 = (unsigned)key;
    k1 = (unsigned)(key >> 32);
}
// per-row words: an offset and an odd 24-bit stride, so that two rows never walk the same hash inputs shifted against each other
__device__ __forceinline__ void vqt_row_words(unsigned n, unsigned k0, unsigned k1, unsigned& off, unsigned& stride) {
    off = dvq_hash32(n ^ k0) + k1;
    stride = (dvq_hash32(n + k1) ^ k0) & 0xffffffu | 1u;
}
// -log(-log(u)), u = (23 random bits + 1/2) * 2^-23 in [2^-24, 1 - 2^-24]: never 0 or 1, so the reference's 1e-20 clamps are inactive
// except for the guard on the inner log.  -ln(-ln u) = -ln(ln 2) - ln 2 * log2(-log2 u).  k < 2^24.
__device__ __forceinline__ float vqt_gumbel(unsigned off, unsigned stride, unsigned k) {
    const unsigned h = dvq_hash32(__umul24(k, stride) + off);
    const float u = ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
    const float t = fmaxf(-__builtin_amdgcn_logf(u), 1e-9f);
    return fmaf(-0.69314718056f, __builtin_amdgcn_logf(t), 0.36651292058f);
}

__global__ __launch_bounds__(256) void vqt_gumbel_noise_kernel(uint64_t seed, uint64_t counter, int64_t N, int64_t K, float* __restrict__ out) {
    unsigned k0, k1;
    vqt_key(seed, counter, k0, k1);
    const int64_t total = N * K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i / K, k = i - n * K;
        unsigned off, stride;
        vqt_row_words((unsigned)n, k0, k1, off, stride);
        out[i] = vqt_gumbel(off, stride, (unsigned)k);
    }
}

__global__ void vqt_bump_state_kernel(uint64_t* state) {
    if (threadIdx.x == 0) state[1] += 1;
}

// Noiseless cosine search: error bound of the DIFFERENCE of two evaluated scores, in cosine units (a_n = 1 / |x_n|, |ê| <= 1): per score
// the split residual 3 * 2^-18, the fp32 accumulation D * 2^-23 (worst case) and 2^-22 for the fp32-normalised code row, the row scale
// and the final multiply; two scores are compared.  A row whose best and second-best score are not further apart is flagged (index
// -1) and vq_cosine_rerank_kernel recomputes ALL its scores in fp64 from the raw codebook: the mathematically exact argmax, lowest index on ties.
__host__ __device__ __forceinline__ float vqt_cos_tau(int64_t D) {
    return 2.0f * (3.0f * 3.8147e-6f + (float)D * 1.1921e-7f + 2.3842e-7f);
}

// ---- search, MFMA path: 4 waves x 32 rows per workgroup, x fragments in registers, the codebook planes stream through LDS in
// 32-code stages (double buffered, register-staged prefetch: the tiling of vq.hip's round-1 kernel).  Lane (l31, half) of a wave owns
// code c * 32 + l31 of stage c for the 16 accumulator rows (r & 3) + 8 (r >> 2) + 4 half: it keeps a running (best value, index) per
// row over ITS codes in ascending order (strict >, so the lowest index survives a tie), and the 32 lanes are merged at the end. ----
template <int KSTEPS, typename XT, bool NOISE, bool COS>
__global__ __launch_bounds__(256, 1) void vq_sample_argmax_mfma_kernel(const XT* __restrict__ x, const void* prep_c, int64_t N, int64_t K,
                                                                       float inv_temp, const uint64_t* __restrict__ state,
                                                                       int64_t* __restrict__ idx_out) {
    constexpr int D = KSTEPS * 16;
    constexpr bool XBF16 = sizeof(XT) == 2;
    constexpr int ROWB = D * 2 + 16;          // LDS bytes per code row (16-B pad -> conflict-free b128 reads)
    constexpr int PIECE = 32 * ROWB;          // one bf16 plane of a 32-code stage
    constexpr int STAGE = 2 * PIECE;
    constexpr int CH_PER_THREAD = D / 64;     // 16-B chunks per thread per plane
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* rscale = reinterpret_cast<float*>(smem + 2 * STAGE);   // [128] per-row scale a_n

    VqtPrep pv = vqt_prep_view(const_cast<void*>(prep_c), K, D);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * 128 + wave * 32;

    // ---- load + split x fragments -------------------------------------------------------------
    bf16x8 xa1[KSTEPS];
    bf16x8 xa2[XBF16 ? 1 : KSTEPS];
    float sq = 0.f;
    {
        const int64_t r = row0 + l31;
        const bool ok = r < N;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            float v[8];
            if (ok) {
                load8(x + r * D + ks * 16 + half * 8, v);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sq = fmaf(v[j], v[j], sq);
                bf16_t h = f32_to_bf16(v[j]);
                xa1[ks][j] = __builtin_bit_cast(__bf16, h);
                if constexpr (!XBF16) {
                    float rr = v[j] - bf16_to_f32(h);
                    xa2[ks][j] = __builtin_bit_cast(__bf16, f32_to_bf16(rr));
                }
            }
        }
    }
    if constexpr (COS) {
        sq += __shfl_xor(sq, 32, 64);
        if (half == 0) rscale[wave * 32 + l31] = inv_temp / fmaxf(sqrtf(sq), 1e-12f);
    }

    // ---- stage loader -------------------------------------------------------------------------
    const int nstage = (int)(pv.Kp / 32);
    uint4 p1_0, p1_1, p1_2, p1_3, p2_0, p2_1, p2_2, p2_3;
    p1_0 = p1_1 = p1_2 = p1_3 = p2_0 = p2_1 = p2_2 = p2_3 = make_uint4(0, 0, 0, 0);
    auto chunk_goff = [&](int i) { const int q = tid + 256 * i; return (q / (D / 8)) * D + (q % (D / 8)) * 8; };
    auto chunk_soff = [&](int i) { const int q = tid + 256 * i; return (q / (D / 8)) * ROWB + (q % (D / 8)) * 16; };
    const int go0 = chunk_goff(0), go1 = chunk_goff(1), go2 = chunk_goff(2), go3 = chunk_goff(3);
    const int so0 = chunk_soff(0), so1 = chunk_soff(1), so2 = chunk_soff(2), so3 = chunk_soff(3);
#define VQT_G1(i, c)                                                                          \
    if constexpr (CH_PER_THREAD > i) {                                                        \
        const int64_t g = (int64_t)(c) * 32 * D + go##i;                                      \
        p1_##i = *reinterpret_cast<const uint4*>(pv.e1 + g);                                  \
        p2_##i = *reinterpret_cast<const uint4*>(pv.e2 + g);                                  \
    }
#define VQT_G_LOAD(c) VQT_G1(0, c) VQT_G1(1, c) VQT_G1(2, c) VQT_G1(3, c)
#define VQT_S1(i, buf)                                                                        \
    if constexpr (CH_PER_THREAD > i) {                                                        \
        char* base = smem + (buf) * STAGE + so##i;                                            \
        *reinterpret_cast<uint4*>(base) = p1_##i;                                             \
        *reinterpret_cast<uint4*>(base + PIECE) = p2_##i;                                     \
    }
#define VQT_S_STORE(buf) VQT_S1(0, buf) VQT_S1(1, buf) VQT_S1(2, buf) VQT_S1(3, buf)

    VQT_G_LOAD(0)
    VQT_S_STORE(0)
    __syncthreads();

    constexpr bool RERANK = COS && !NOISE;       // noiseless cosine: rows whose two best scores are not separated are settled in fp64
    float best[16], arow[16], b2[RERANK ? 16 : 1];
    int bi[16];
    unsigned noff[16], nstr[16];
    unsigned k0 = 0, k1 = 0;
    if constexpr (NOISE) vqt_key(state[0], state[1], k0, k1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * half;
        best[r] = -__builtin_inff();
        if constexpr (RERANK) b2[r] = -__builtin_inff();
        bi[r] = 0x7fffffff;
        arow[r] = COS ? rscale[wave * 32 + rl] : 2.0f * inv_temp;
        if constexpr (NOISE) vqt_row_words((unsigned)(row0 + rl), k0, k1, noff[r], nstr[r]);
    }

    for (int c = 0; c < nstage; ++c) {
        const int buf = c & 1;
        if (c + 1 < nstage) {
            VQT_G_LOAD(c + 1)
        }
        const int kidx = c * 32 + l31;
        const float bk = pv.bias[kidx] * inv_temp;
        f32x16 acc_hi = {0}, acc_lo = {0};
        const char* bbase = smem + buf * STAGE + l31 * ROWB + half * 16;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            bf16x8 e1f = *reinterpret_cast<const bf16x8*>(bbase + ks * 32);
            bf16x8 e2f = *reinterpret_cast<const bf16x8*>(bbase + PIECE + ks * 32);
            acc_hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa1[ks], e1f, acc_hi, 0, 0, 0);
            acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa1[ks], e2f, acc_lo, 0, 0, 0);
            if constexpr (!XBF16) acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa2[ks], e1f, acc_lo, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = fmaf(arow[r], acc_hi[r] + acc_lo[r], bk);
            if constexpr (NOISE) v += vqt_gumbel(noff[r], nstr[r], (unsigned)kidx);
            const bool gt = v > best[r];
            if constexpr (RERANK) b2[r] = gt ? best[r] : fmaxf(b2[r], v);
            bi[r] = gt ? kidx : bi[r];
            best[r] = gt ? v : best[r];
        }
        if (c + 1 < nstage) {
            VQT_S_STORE(buf ^ 1)
        }
        __syncthreads();
    }
#undef VQT_G_LOAD
#undef VQT_S_STORE
#undef VQT_G1
#undef VQT_S1

#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float gb = best[r], g2 = RERANK ? b2[r] : 0.f;
        int gi = bi[r];
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const float ob = __shfl_xor(gb, o, 64);
            const int oi = __shfl_xor(gi, o, 64);
            const bool take = (ob > gb) || (ob == gb && oi < gi);
            if constexpr (RERANK) g2 = fmaxf(fmaxf(g2, __shfl_xor(g2, o, 64)), take ? gb : ob);      // the second best of both halves
            gb = take ? ob : gb;
            gi = take ? oi : gi;
        }
        const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        int64_t res = gi < K ? (int64_t)gi : 0;      // a row of NaNs beats nothing: index 0, never out of range
        if constexpr (RERANK) {
            if (!(gb - g2 > vqt_cos_tau(D))) res = -1;      // flagged: vq_cosine_rerank_kernel settles it (exact ties included)
        }
        if (l31 == 0 && row < N) idx_out[row] = res;
    }
}

// ---- search, generic path (any D): one wave per row, a lane per code (k = lane, lane + 64, ...), fp32 FMA dot products over the two
// prepared planes (e1 + e2 is e to 2^-17).  Correct rather than fast. ----
template <typename XT>
__global__ __launch_bounds__(256) void vq_sample_argmax_generic_kernel(const XT* __restrict__ x, const void* prep_c, int64_t N, int64_t K,
                                                                       int64_t D, int cosine, int noise, float inv_temp,
                                                                       const uint64_t* __restrict__ state, int64_t* __restrict__ idx_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xs = reinterpret_cast<float*>(smem) + (threadIdx.x >> 6) * D;
    VqtPrep pv = vqt_prep_view(const_cast<void*>(prep_c), K, D);
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    float sq = 0.f;
    if (n < N) {
        for (int64_t d = lane; d < D; d += 64) {
            const float v = ElemIO<XT>::load(x + n * D + d);
            xs[d] = v;
            sq = fmaf(v, v, sq);
        }
    }
    __syncthreads();
    if (n >= N) return;
    sq = wave_sum(sq);
    const float a = cosine ? inv_temp / fmaxf(sqrtf(sq), 1e-12f) : 2.0f * inv_temp;
    unsigned off = 0, stride = 1;
    if (noise) {
        unsigned k0, k1;
        vqt_key(state[0], state[1], k0, k1);
        vqt_row_words((unsigned)n, k0, k1, off, stride);
    }
    const bool rerank = cosine && !noise;
    float gb = -__builtin_inff(), g2 = -__builtin_inff();
    int gi = 0x7fffffff;
    for (int64_t k = lane; k < K; k += 64) {
        const bf16_t* e1 = pv.e1 + k * D;
        const bf16_t* e2 = pv.e2 + k * D;
        float dot = 0.f;
        for (int64_t d = 0; d < D; ++d) dot = fmaf(xs[d], bf16_to_f32(e1[d]) + bf16_to_f32(e2[d]), dot);
        float v = fmaf(a, dot, pv.bias[k] * inv_temp);
        if (noise) v += vqt_gumbel(off, stride, (unsigned)k);
        if (v > gb) {
            g2 = gb;
            gb = v;
            gi = (int)k;
        } else {
            g2 = fmaxf(g2, v);
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ob = __shfl_xor(gb, o, 64);
        const int oi = __shfl_xor(gi, o, 64);
        const bool take = (ob > gb) || (ob == gb && oi < gi);
        g2 = fmaxf(fmaxf(g2, __shfl_xor(g2, o, 64)), take ? gb : ob);
        gb = take ? ob : gb;
        gi = take ? oi : gi;
    }
    int64_t res = gi < K ? (int64_t)gi : 0;
    if (rerank && !(gb - g2 > vqt_cos_tau(D))) res = -1;
    if (lane == 0) idx_out[n] = res;
}

// ---- fp64 re-rank of the rows the noiseless cosine search flagged (index -1): one wave per row, a lane per code, cosine similarity from
// the RAW codebook in fp64 (the row's own positive norm does not change its argmax), lowest index on ties; an all-zero row scores 0
// against every code: index 0.  Rare rows (a per cent at K = 1024, D = 256), so plain loads. ----
template <typename XT>
__global__ __launch_bounds__(256) void vq_cosine_rerank_kernel(const XT* __restrict__ x, const float* __restrict__ cb, int64_t N, int64_t K,
                                                               int64_t D, int64_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N || idx[n] >= 0) return;          // wave-uniform
    double gb = -__builtin_inf();
    int gi = 0x7fffffff;
    for (int64_t k = lane; k < K; k += 64) {
        double dot = 0.0, en = 0.0;
        for (int64_t d = 0; d < D; ++d) {
            const double e = (double)cb[k * D + d];
            dot = fma((double)ElemIO<XT>::load(x + n * D + d), e, dot);
            en = fma(e, e, en);
        }
        const double c = dot / fmax(sqrt(en), 1e-12);
        if (c > gb) {
            gb = c;
            gi = (int)k;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double ob = __shfl_xor(gb, o, 64);
        const int oi = __shfl_xor(gi, o, 64);
        const bool take = (ob > gb) || (ob == gb && oi < gi);
        gb = take ? ob : gb;
        gi = take ? oi : gi;
    }
    if (lane == 0) idx[n] = gi < K ? (int64_t)gi : 0;
}

// ---- codebook gradient: one wave per (code k, slice of CG_SLICE rows), the walk of vq_ema_stats_kernel: the slice's indices are
// scanned 64 at a time with unconditional (clamped) loads, the matching rows form a compact list in slice order, the list is walked
// four rows per trip.  Work per wave is bounded by the slice however skewed the code usage is.  ALL = false: grid.y slices, one fp32
// atomic per dimension per (code, slice).  ALL = true (deterministic mode): ONE wave per code walks every slice in order and adds its
// sum to the gradient with a plain read-modify-write (no other wave touches row k): bit-identical launch to launch. ----
constexpr int CG_SLICE = 1024;

template <typename T, int NJ, bool ALL>
__global__ __launch_bounds__(64) void vq_codebook_grad_kernel(const T* __restrict__ x, const float* __restrict__ cb,
                                                              const int64_t* __restrict__ idx, const float* __restrict__ mask,
                                                              const float* __restrict__ coef_dev, int64_t N, int64_t K, int64_t D,
                                                              float* __restrict__ grad) {
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    constexpr int NCH = CG_SLICE / 64;
    __shared__ unsigned short rows_l[CG_SLICE];
    const int64_t nslices = (N + CG_SLICE - 1) / CG_SLICE;
    const int64_t s_beg = ALL ? 0 : blockIdx.y, s_end = ALL ? nslices : (int64_t)blockIdx.y + 1;
    float acc[NJ], ek[NJ];
    int dj[NJ];                                  // this lane's columns, clamped into the row (masked when past D)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        acc[j] = 0.f;
        dj[j] = (int)min((int64_t)(lane + 64 * j), D - 1);
        ek[j] = cb[k * D + dj[j]];
    }
    bool any = false;
    for (int64_t sl = s_beg; sl < s_end; ++sl) {
        const int64_t nbeg = sl * CG_SLICE, nend = min(N, nbeg + CG_SLICE);
        int64_t iv[NCH];
#pragma unroll
        for (int q = 0; q < NCH; ++q) iv[q] = idx[min(nbeg + q * 64 + lane, N - 1)];
        unsigned long long hit[NCH];
        int count = 0;
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            hit[q] = __ballot(nbeg + q * 64 + lane < nend && iv[q] == k);
            count += __popcll(hit[q]);
        }
        if (count == 0) continue;               // wave-uniform
        any = true;
        __syncthreads();                          // the previous slice's list is no longer read
        {
            int base = 0;
#pragma unroll
            for (int q = 0; q < NCH; ++q) {
                const unsigned long long below = hit[q] & ((1ull << lane) - 1ull);
                if ((hit[q] >> lane) & 1ull) rows_l[base + __popcll(below)] = (unsigned short)(q * 64 + lane);
                base += __popcll(hit[q]);
            }
        }
        __syncthreads();
        for (int i = 0; i < count; i += 4) {
            float v[4][NJ], m[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t n = nbeg + rows_l[min(i + u, count - 1)];
                const T* row = x + n * D;
                m[u] = mask != nullptr ? mask[n] : 1.0f;
#pragma unroll
                for (int j = 0; j < NJ; ++j) v[u][j] = ElemIO<T>::load(row + dj[j]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float mu = i + u < count ? m[u] : 0.f;
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = fmaf(mu, ek[j] - v[u][j], acc[j]);
            }
        }
    }
    if (!any) return;
    const float c = coef_dev[0];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t d = lane + 64 * j;
        if (d < D) {
            if constexpr (ALL) grad[k * D + d] += c * acc[j];
            else atomicAdd(grad + k * D + d, c * acc[j]);
        }
    }
}

// ---- N / sum(mask): one workgroup, fixed summation order ----
__global__ __launch_bounds__(256) void vq_mask_ratio_kernel(const float* __restrict__ mask, int64_t N, float* __restrict__ out) {
    __shared__ double part[256];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) a += (double)mask[i];
    part[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)((double)N / part[0]);
}

// ---- orthogonality regulariser: W = normalize(E), G = W W^T - I, term = sum G^2 (the caller scales by w / K^2) ----
// one wave per code: W[k,:] = E[k,:] / max(|E[k,:]|, 1e-12), inv[k] = that reciprocal
__global__ __launch_bounds__(256) void vq_rownorm_kernel(const float* __restrict__ e, int64_t K, int64_t D, float* __restrict__ w,
                                                         float* __restrict__ inv) {
    const int64_t k = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (k >= K) return;
    float a = 0.f;
    for (int64_t d = lane; d < D; d += 64) a = fmaf(e[k * D + d], e[k * D + d], a);
    a = wave_sum(a);
    const float r = 1.0f / fmaxf(sqrtf(a), 1e-12f);
    for (int64_t d = lane; d < D; d += 64) w[k * D + d] = e[k * D + d] * r;
    if (lane == 0) inv[k] = r;
}
// G[i,j] -= (i == j) in place, one partial sum of G^2 per workgroup (fixed order), folded by the last kernel below
__global__ __launch_bounds__(256) void vq_ortho_sumsq_kernel(float* __restrict__ g, int64_t K, double* __restrict__ partial) {
    __shared__ double part[256];
    double a = 0.0;
    const int64_t total = K * K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / K, c = i - r * K;
        const float v = g[i] - (r == c ? 1.0f : 0.0f);
        g[i] = v;
        a += (double)v * (double)v;
    }
    part[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = part[0];
}
__global__ __launch_bounds__(256) void vq_ortho_fold_kernel(const double* __restrict__ partial, int n, float scale, float* __restrict__ out) {
    __shared__ double part[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
    part[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(part[0] * (double)scale);
}
// backward of the normalisation, accumulated: grad[k,:] += c * scale * (dW[k,:] - W[k,:] (W[k,:] . dW[k,:])) * inv[k]
__global__ __launch_bounds__(256) void vq_rownorm_bwd_kernel(const float* __restrict__ w, const float* __restrict__ inv,
                                                             const float* __restrict__ dw, const float* __restrict__ coef_dev, float scale,
                                                             int64_t K, int64_t D, float* __restrict__ grad) {
    const int64_t k = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (k >= K) return;
    float a = 0.f;
    for (int64_t d = lane; d < D; d += 64) a = fmaf(w[k * D + d], dw[k * D + d], a);
    a = wave_sum(a);
    const float c = coef_dev[0] * scale * inv[k];
    for (int64_t d = lane; d < D; d += 64) grad[k * D + d] += c * (dw[k * D + d] - w[k * D + d] * a);
}

constexpr int ORTHO_BLOCKS = 256;

}  // namespace

// =================================================================================================
extern "C" {

size_t dvq_vq_trained_prep_bytes(int64_t K, int64_t D) {
    const int64_t Kp = vqt_align_up(K, 32);
    return (size_t)(vqt_align_up(Kp * 4, 256) + 2 * Kp * D * 2);
}

int dvq_vq_trained_prepare(const float* codebook, int64_t K, int64_t D, int cosine, void* prep, dvq_stream_t stream) {
    DVQ_REQUIRE(codebook && prep && K > 0 && D > 0, DVQ_EINVAL, "dvq_vq_trained_prepare: bad arguments");
    const int64_t Kp = vqt_align_up(K, 32);
    vqt_prepare_kernel<<<dim3((unsigned)cdiv64(Kp, 4)), dim3(256), 0, (hipStream_t)stream>>>(codebook, K, D, cosine, prep);
    DVQ_CHECK_LAUNCH("vqt_prepare");
    return DVQ_OK;
}

int dvq_vq_sample_argmax(const void* x, int x_dtype, const void* prep, const float* codebook, int64_t N, int64_t K, int64_t D, int cosine,
                         float temp, uint64_t* state, int64_t* idx, dvq_stream_t stream) {
    DVQ_REQUIRE(x && prep && idx, DVQ_EINVAL, "dvq_vq_sample_argmax: null pointer");
    DVQ_REQUIRE(!(cosine && temp == 0.f) || codebook, DVQ_EINVAL, "dvq_vq_sample_argmax: the noiseless cosine search needs the raw codebook (fp64 re-rank)");
    DVQ_REQUIRE(x_dtype == DVQ_F32 || x_dtype == DVQ_BF16, DVQ_EINVAL, "dvq_vq_sample_argmax: bad dtype %d", x_dtype);
    DVQ_REQUIRE(N > 0 && K > 0 && D > 0 && N < (1ll << 31) && K < (1ll << 24) && D <= 4096, DVQ_ESHAPE,
                "dvq_vq_sample_argmax: bad shape N=%lld K=%lld D=%lld (N < 2^31, K < 2^24, D <= 4096)", (long long)N, (long long)K, (long long)D);
    DVQ_REQUIRE(temp >= 0.f, DVQ_EINVAL, "dvq_vq_sample_argmax: temp < 0");
    const bool noise = temp > 0.f;
    DVQ_REQUIRE(!noise || state, DVQ_EINVAL, "dvq_vq_sample_argmax: temp > 0 needs the device {seed, counter} state");
    const float inv_temp = noise ? 1.0f / temp : 1.0f;
    hipStream_t s = (hipStream_t)stream;
    if (D == 64 || D == 128 || D == 256) {
        dvq_note_kernel("vq_sample_argmax_mfma_kernel");
        const dim3 grid((unsigned)cdiv64(N, 128)), block(256);
        auto launch = [&](auto ksteps, auto xt, auto nz, auto cs) {
            constexpr int KS = decltype(ksteps)::value;
            using XT = decltype(xt);
            constexpr bool NZ = decltype(nz)::value, CS = decltype(cs)::value;
            const size_t lds = 2 * (2 * 32 * (KS * 16 * 2 + 16)) + 128 * 4;
            dvq_ensure_dynamic_lds((const void*)vq_sample_argmax_mfma_kernel<KS, XT, NZ, CS>, (int)lds);
            vq_sample_argmax_mfma_kernel<KS, XT, NZ, CS><<<grid, block, lds, s>>>((const XT*)x, prep, N, K, inv_temp, state, idx);
        };
        auto by_flags = [&](auto ksteps, auto xt) {
            if (noise && cosine) launch(ksteps, xt, std::true_type{}, std::true_type{});
            else if (noise) launch(ksteps, xt, std::true_type{}, std::false_type{});
            else if (cosine) launch(ksteps, xt, std::false_type{}, std::true_type{});
            else launch(ksteps, xt, std::false_type{}, std::false_type{});
        };
        auto by_dtype = [&](auto ksteps) {
            if (x_dtype == DVQ_F32) by_flags(ksteps, float{});
            else by_flags(ksteps, bf16_t{});
        };
        if (D == 64) by_dtype(std::integral_constant<int, 4>{});
        else if (D == 128) by_dtype(std::integral_constant<int, 8>{});
        else by_dtype(std::integral_constant<int, 16>{});
        DVQ_CHECK_LAUNCH("vq_sample_argmax_mfma");
    } else {
        dvq_note_kernel("vq_sample_argmax_generic_kernel");
        const size_t lds = 4 * (size_t)D * 4;
        DVQ_DISPATCH_DTYPE(x_dtype, T, vq_sample_argmax_generic_kernel<T><<<dim3((unsigned)cdiv64(N, 4)), dim3(256), lds, s>>>(
                                           (const T*)x, prep, N, K, D, cosine, noise ? 1 : 0, inv_temp, state, idx););
        DVQ_CHECK_LAUNCH("vq_sample_argmax_generic");
    }
    if (noise) {
        vqt_bump_state_kernel<<<dim3(1), dim3(64), 0, s>>>(state);
        DVQ_CHECK_LAUNCH("vqt_bump_state");
    } else if (cosine) {
        DVQ_DISPATCH_DTYPE(x_dtype, T, vq_cosine_rerank_kernel<T><<<dim3((unsigned)cdiv64(N, 4)), dim3(256), 0, s>>>((const T*)x, codebook, N, K, D, idx););
        DVQ_CHECK_LAUNCH("vq_cosine_rerank");
    }
    return DVQ_OK;
}

int dvq_vq_gumbel_noise(uint64_t seed, uint64_t counter, int64_t N, int64_t K, float* out, dvq_stream_t stream) {
    DVQ_REQUIRE(out && N > 0 && K > 0 && N < (1ll << 31) && K < (1ll << 24), DVQ_EINVAL, "dvq_vq_gumbel_noise: bad arguments");
    int64_t blocks = cdiv64(N * K, 256);
    if (blocks > 4096) blocks = 4096;
    vqt_gumbel_noise_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(seed, counter, N, K, out);
    DVQ_CHECK_LAUNCH("vqt_gumbel_noise");
    return DVQ_OK;
}

int dvq_vq_codebook_grad(const void* x, int dtype, const float* codebook, const int64_t* idx, const float* mask, const float* coef_dev,
                         int64_t N, int64_t K, int64_t D, float* grad, dvq_stream_t stream) {
    DVQ_REQUIRE(x && codebook && idx && coef_dev && grad, DVQ_EINVAL, "dvq_vq_codebook_grad: null pointer");
    DVQ_REQUIRE(dtype == DVQ_F32 || dtype == DVQ_BF16, DVQ_EINVAL, "dvq_vq_codebook_grad: bad dtype %d", dtype);
    DVQ_REQUIRE(N > 0 && K > 0 && D > 0 && D <= 1024 && K < (1ll << 31), DVQ_ESHAPE, "dvq_vq_codebook_grad: bad shape (D <= 1024)");
    hipStream_t s = (hipStream_t)stream;
    const bool all = dvq_deterministic() != 0;
    const dim3 grid((unsigned)K, all ? 1u : (unsigned)cdiv64(N, CG_SLICE));
    DVQ_REQUIRE(cdiv64(N, CG_SLICE) <= 65535, DVQ_ESHAPE, "dvq_vq_codebook_grad: N too large");
#define DVQ_CB_GRAD(NJV)                                                                                                             \
    DVQ_DISPATCH_DTYPE(dtype, T,                                                                                                     \
                       if (all) vq_codebook_grad_kernel<T, NJV, true><<<grid, dim3(64), 0, s>>>((const T*)x, codebook, idx, mask, coef_dev, N, K, D, grad); \
                       else vq_codebook_grad_kernel<T, NJV, false><<<grid, dim3(64), 0, s>>>((const T*)x, codebook, idx, mask, coef_dev, N, K, D, grad);)
    if (D <= 64) { DVQ_CB_GRAD(1); } else if (D <= 128) { DVQ_CB_GRAD(2); } else if (D <= 256) { DVQ_CB_GRAD(4); }
    else if (D <= 512) { DVQ_CB_GRAD(8); } else { DVQ_CB_GRAD(16); }
#undef DVQ_CB_GRAD
    DVQ_CHECK_LAUNCH("vq_codebook_grad");
    return DVQ_OK;
}

int dvq_vq_mask_ratio(const float* mask, int64_t N, float* out, dvq_stream_t stream) {
    DVQ_REQUIRE(mask && out && N > 0, DVQ_EINVAL, "dvq_vq_mask_ratio: bad arguments");
    vq_mask_ratio_kernel<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>(mask, N, out);
    DVQ_CHECK_LAUNCH("vq_mask_ratio");
    return DVQ_OK;
}

int dvq_vq_rownorm(const float* e, int64_t K, int64_t D, float* w, float* inv, dvq_stream_t stream) {
    DVQ_REQUIRE(e && w && inv && K > 0 && D > 0, DVQ_EINVAL, "dvq_vq_rownorm: bad arguments");
    vq_rownorm_kernel<<<dim3((unsigned)cdiv64(K, 4)), dim3(256), 0, (hipStream_t)stream>>>(e, K, D, w, inv);
    DVQ_CHECK_LAUNCH("vq_rownorm");
    return DVQ_OK;
}

size_t dvq_vq_ortho_scratch_bytes(void) { return ORTHO_BLOCKS * sizeof(double); }

int dvq_vq_ortho_sumsq(float* g, int64_t K, float scale, void* scratch, float* out, dvq_stream_t stream) {
    DVQ_REQUIRE(g && scratch && out && K > 0, DVQ_EINVAL, "dvq_vq_ortho_sumsq: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    vq_ortho_sumsq_kernel<<<dim3(ORTHO_BLOCKS), dim3(256), 0, s>>>(g, K, (double*)scratch);
    DVQ_CHECK_LAUNCH("vq_ortho_sumsq");
    vq_ortho_fold_kernel<<<dim3(1), dim3(256), 0, s>>>((const double*)scratch, ORTHO_BLOCKS, scale, out);
    DVQ_CHECK_LAUNCH("vq_ortho_fold");
    return DVQ_OK;
}

int dvq_vq_rownorm_bwd(const float* w, const float* inv, const float* dw, const float* coef_dev, float scale, int64_t K, int64_t D,
                       float* grad, dvq_stream_t stream) {
    DVQ_REQUIRE(w && inv && dw && coef_dev && grad && K > 0 && D > 0, DVQ_EINVAL, "dvq_vq_rownorm_bwd: bad arguments");
    vq_rownorm_bwd_kernel<<<dim3((unsigned)cdiv64(K, 4)), dim3(256), 0, (hipStream_t)stream>>>(w, inv, dw, coef_dev, scale, K, D, grad);
    DVQ_CHECK_LAUNCH("vq_rownorm_bwd");
    return DVQ_OK;
}

}  // extern "C"
