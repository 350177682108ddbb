// Lossless token codec of the DQ-Transformer (gfx950; docs/design/27-token-codec.md).  No counterpart in the reference.
//
// A logits row becomes an integer frequency table (codec_table, the ONE function encoder and decoder share):
//   allowed set A = the columns the token rule (dvq_token_rule of include/dvq_hip.h, applied by token_rule.h: the sampler's code) leaves
//                   unmasked; in a live row the logit must be finite as well;  n = |A|
//   n == 1:  f = M on that column (nothing is coded);  n == 0: all zero (an error for the callers)
//   n >= 2:  e_c = expf(x_c - max_A x);  S = sum_A e_c in fp32: lane l adds its columns l, l + 64, ... in ascending order, then the xor
//            tree of wave_sum;  f_c = 1 + floor(e_c / S * (M - n));  the exact integer remainder M - sum f goes to the lowest-index
//            arg-max column (it stays >= 1 for n <= DVQ_TOKEN_RULE_MAXV: the design note has the argument);  M = 2^16
// so sum f = M, f >= 1 on A, f = 0 elsewhere; cum_c = exclusive prefix sum in column order.
// The coder is rANS with a 64-bit state, lower bound L = 2^31, 32-bit words and 16-bit frequencies: a symbol emits at most one word.
// dvq_codec_record stores (cum, f) of the target per step; dvq_codec_encode walks an image's records backwards and writes its words
// from the END of its buffer, so dvq_codec_decode_step reads them forwards.
// One wave per row.  Every output element is written by one lane with a plain store: no atomics.  The error words are one per row.
#include "dvq_common.h"
#include "token_rule.h"

#include <math.h>

namespace {

constexpr unsigned CODEC_M = 1u << 16;
constexpr uint64_t CODEC_L = 1ull << 31;
constexpr int CODEC_MAXV = DVQ_TOKEN_RULE_MAXV;
constexpr int CODEC_NI = CODEC_MAXV / 64;        // columns per lane, lane-strided (the softmax) and contiguous (the prefix sums)
constexpr int CODEC_LDS = CODEC_MAXV + CODEC_MAXV / 32;

struct CodecParams {
    const void* logits;
    int64_t ldl;
    int V;
    TokenRule rule;
};

struct CodecTable {
    bool fin;               // a finished row: the token is pad_code, nothing is coded
    int n;                  // |A|
    int amax;               // lowest-index arg-max column of A (n == 1: the one allowed column)
    unsigned base, tot;     // this lane's contiguous columns [32 lane, 32 lane + 32): cum of the first one, sum of their f
};

// column c of the table in LDS: one pad word per 32 columns, so that lanes walking their 32 contiguous columns hit distinct banks
__device__ __forceinline__ int codec_slot(int c) { return c + (c >> 5); }

template <typename T>
__device__ __forceinline__ CodecTable codec_table(const CodecParams& p, int row, unsigned* __restrict__ sf, unsigned char* __restrict__ flag) {
    const int lane = threadIdx.x, V = p.V;
    CodecTable t;
    t.fin = token_rule_finished(p.rule, row);
    token_rule_mark(p.rule, t.fin, row, V, flag, V, lane, 64);
    const T* lg = reinterpret_cast<const T*>(p.logits) + (int64_t)row * p.ldl;
    float x[CODEC_NI];
    float m = -INFINITY;
    int cnt = 0;
    unsigned okmask = 0;                             // bit i: column lane + 64 i is in A
#pragma unroll
    for (int i = 0; i < CODEC_NI; ++i) {
        x[i] = -INFINITY;
        const int c = lane + 64 * i;
        if (c < V) {
            bool ok;
            float v = 0.f;
            if (t.fin) {
                ok = !token_rule_masked(p.rule, true, flag, c);
            } else {                                                         // A of a live row: not masked AND a finite logit
                v = ElemIO<T>::load(lg + c);
                ok = !token_rule_masked(p.rule, false, flag, c) && v > -INFINITY && v < INFINITY;       // (NaN fails both comparisons)
            }
            if (ok) {
                x[i] = v;
                m = fmaxf(m, v);
                ++cnt;
                okmask |= 1u << i;
            }
        }
    }
    m = wave_max(m);
    t.n = wave_sum(cnt);
    int am = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < CODEC_NI; ++i)
        if (((okmask >> i) & 1u) && x[i] == m) am = min(am, lane + 64 * i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
    t.amax = t.n > 0 ? am : 0;
    int fsum = 0;
    if (t.n >= 2) {
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < CODEC_NI; ++i) {
            x[i] = ((okmask >> i) & 1u) ? expf(x[i] - m) : 0.f;          // (may underflow to 0: f = 1)
            part += x[i];
        }
        const float S = wave_sum(part);
        const float scale = (float)(CODEC_M - (unsigned)t.n);
#pragma unroll
        for (int i = 0; i < CODEC_NI; ++i) {
            const int c = lane + 64 * i;
            if (c < V) {
                const unsigned f = ((okmask >> i) & 1u) ? 1u + (unsigned)floorf(x[i] / S * scale) : 0u;
                sf[codec_slot(c)] = f;
                fsum += (int)f;
            }
        }
    } else {
        for (int c = lane; c < V; c += 64) sf[codec_slot(c)] = (t.n == 1 && c == t.amax) ? CODEC_M : 0u;
    }
    fsum = wave_sum(fsum);
    __syncthreads();
    if (t.n >= 2 && lane == 0) sf[codec_slot(t.amax)] = (unsigned)((int)sf[codec_slot(t.amax)] + ((int)CODEC_M - fsum));
    __syncthreads();
    // exclusive prefix sums in column order: lane l owns columns [32 l, 32 l + 32)
    unsigned tot = 0;
    const int c0 = lane * 32;
    for (int c = c0; c < min(V, c0 + 32); ++c) tot += sf[codec_slot(c)];
    unsigned incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    t.base = incl - tot;
    t.tot = tot;
    return t;
}

enum { CODEC_ERR_TARGET = 1, CODEC_ERR_UNDERRUN = 2, CODEC_ERR_EMPTY = 4, CODEC_ERR_SEARCH = 8 };

template <typename T>
__global__ __launch_bounds__(64) void codec_tables_kernel(CodecParams p, uint32_t* __restrict__ out) {
    __shared__ unsigned sf[CODEC_LDS];
    __shared__ unsigned char flag[CODEC_MAXV];
    const int row = blockIdx.x;
    codec_table<T>(p, row, sf, flag);
    for (int c = threadIdx.x; c < p.V; c += 64) out[(int64_t)row * p.V + c] = sf[codec_slot(c)];
}

// a record: cum | f << 16 (f in [1, 65535]); 0 = nothing coded at this step
template <typename T>
__global__ __launch_bounds__(64) void codec_record_kernel(CodecParams p, const int64_t* __restrict__ target, uint32_t* __restrict__ records,
                                                          int64_t rec_ld, int64_t step, int64_t* __restrict__ token,
                                                          uint32_t* __restrict__ err) {
    __shared__ unsigned sf[CODEC_LDS];
    __shared__ unsigned char flag[CODEC_MAXV];
    const int row = blockIdx.x, lane = threadIdx.x;
    const CodecTable t = codec_table<T>(p, row, sf, flag);
    const int64_t tg = target[row];
    const bool in_range = tg >= 0 && tg < p.V;
    uint32_t rec = 0, e = 0;
    if (!t.fin) {
        if (t.n == 0) e |= CODEC_ERR_EMPTY;
        const unsigned f = in_range ? sf[codec_slot((int)tg)] : 0u;
        if (f == 0) {
            e |= CODEC_ERR_TARGET;
        } else if (t.n >= 2) {
            const int owner = (int)tg >> 5;
            unsigned cum = t.base;
            if (lane == owner)
                for (int c = owner * 32; c < (int)tg; ++c) cum += sf[codec_slot(c)];
            cum = __shfl(cum, owner, 64);
            rec = cum | (f << 16);
        }
    }
    if (lane == 0) {
        records[(int64_t)row * rec_ld + step] = rec;
        token[row] = t.fin || !in_range ? (int64_t)p.rule.pad_code : tg;
        if (e) err[row] |= e;
    }
}

// per-row decoder state, int64 [B][4]: {rANS state, cursor, first word of the row's stream in `words`, number of words of the stream}
template <typename T>
__global__ __launch_bounds__(64) void codec_decode_kernel(CodecParams p, int64_t* __restrict__ state, const uint32_t* __restrict__ words,
                                                          int64_t total_words, int64_t* __restrict__ token, uint32_t* __restrict__ err) {
    __shared__ unsigned sf[CODEC_LDS];
    __shared__ unsigned char flag[CODEC_MAXV];
    const int row = blockIdx.x, lane = threadIdx.x;
    const CodecTable t = codec_table<T>(p, row, sf, flag);
    int64_t tok = p.rule.pad_code;
    uint32_t e = 0;
    if (!t.fin) {
        if (t.n == 0) {
            e |= CODEC_ERR_EMPTY;
        } else if (t.n == 1) {
            tok = t.amax;
        } else {
            int64_t* st = state + (int64_t)row * 4;
            uint64_t x = (uint64_t)st[0];
            const unsigned slot = (unsigned)(x & (CODEC_M - 1));
            // the lane whose contiguous columns cover `slot`, then a walk over at most 32 columns
            const bool mine = slot >= t.base && slot < t.base + t.tot;
            int col = 0;
            unsigned cum = t.base, f = 0;
            if (mine) {
                const int c0 = lane * 32;
                for (int c = c0; c < min(p.V, c0 + 32); ++c) {
                    f = sf[codec_slot(c)];
                    if (slot < cum + f) {
                        col = c;
                        break;
                    }
                    cum += f;
                }
            }
            const unsigned long long who = __ballot(mine);
            if (who == 0) {
                e |= CODEC_ERR_SEARCH;                                 // (sum f = M: cannot happen)
            } else {
                const int owner = __ffsll((long long)who) - 1;
                col = __shfl(col, owner, 64);
                cum = __shfl(cum, owner, 64);
                f = __shfl(f, owner, 64);
                tok = col;
                if (lane == 0) {
                    x = (uint64_t)f * (x >> 16) + slot - cum;
                    if (x < CODEC_L) {
                        const int64_t cur = st[1], at = st[2] + cur;
                        uint32_t w = 0;
                        if (cur >= 0 && cur < st[3] && at >= 0 && at < total_words) {
                            w = words[at];
                            st[1] = cur + 1;
                        } else {
                            e |= CODEC_ERR_UNDERRUN;                   // a read past the stream yields zero: never outside the buffer
                        }
                        x = (x << 32) | w;
                    }
                    st[0] = (int64_t)x;
                }
            }
        }
    }
    if (lane == 0) {
        token[row] = tok;
        if (e) err[row] |= e;
    }
}

constexpr int CODEC_STAGE = 1024;

// one wave per image: lane 0 codes the records last to first (staged through LDS 1024 at a time); all lanes add the ideal bits
// 16 - log2 f per stream in fp64, lane-strided, then the fixed tree of wave_sum
__global__ __launch_bounds__(64) void codec_encode_kernel(const uint32_t* __restrict__ records, int64_t rec_ld, int64_t T,
                                                          const int64_t* __restrict__ counts, const uint8_t* __restrict__ kinds,
                                                          uint32_t* __restrict__ words, int64_t cap, int64_t* __restrict__ nwords,
                                                          double* __restrict__ bits) {
    __shared__ uint32_t buf[CODEC_STAGE];
    const int row = blockIdx.x, lane = threadIdx.x;
    const uint32_t* rec = records + (int64_t)row * rec_ld;
    int64_t cnt = counts != nullptr ? counts[row] : T;
    cnt = cnt < 0 ? 0 : cnt > T ? T : cnt;
    uint32_t* const end = words + (int64_t)row * cap + cap;
    uint32_t* wp = end;
    uint64_t x = CODEC_L;
    for (int64_t hi = cnt; hi > 0; hi -= CODEC_STAGE) {
        const int64_t lo = hi > CODEC_STAGE ? hi - CODEC_STAGE : 0;
        for (int64_t s = lo + lane; s < hi; s += 64) buf[s - lo] = rec[s];
        __syncthreads();
        if (lane == 0)
            for (int64_t s = hi - 1; s >= lo; --s) {
                const uint32_t r = buf[s - lo];
                const uint64_t f = r >> 16, cum = r & 0xffffu;
                if (f == 0) continue;
                if (x >= (f << 47)) {                                  // ((L >> 16) << 32) * f
                    *--wp = (uint32_t)x;
                    x >>= 32;
                }
                x = ((x / f) << 16) + (x % f) + cum;
            }
        __syncthreads();
    }
    if (lane == 0) {                                                   // at most cnt + 2 <= cap words
        *--wp = (uint32_t)(x >> 32);
        *--wp = (uint32_t)x;
        nwords[row] = (int64_t)(end - wp);
    }
    if (bits != nullptr) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t s = lane; s < cnt; s += 64) {
            const uint32_t f = rec[s] >> 16;
            const int k = kinds != nullptr ? kinds[s] : 0;
            if (f != 0 && k < 3) acc[k] += 16.0 - log2((double)f);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = wave_sum(acc[k]);
            if (lane == 0) bits[(int64_t)row * 3 + k] = v;
        }
    }
}

// the logits arguments and the rule that the three row kernels share; false on a bad one
bool codec_params(CodecParams& p, const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, const dvq_token_rule* rule) {
    if (!(logits && ldl >= V && (dtype == DVQ_F32 || dtype == DVQ_BF16) && token_rule_fill(p.rule, rule, B, V))) return false;
    p.logits = logits; p.ldl = ldl; p.V = (int)V;
    return true;
}

}  // namespace

int dvq_codec_tables(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, const dvq_token_rule* rule, uint32_t* table,
                     dvq_stream_t stream) {
    CodecParams p{};
    DVQ_REQUIRE(table && codec_params(p, logits, dtype, B, V, ldl, rule), DVQ_EINVAL, "dvq_codec_tables: bad arguments (V <= %d)",
                CODEC_MAXV);
    DVQ_DISPATCH_DTYPE(dtype, TT, codec_tables_kernel<TT><<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(p, table););
    DVQ_CHECK_LAUNCH("codec_tables");
    return DVQ_OK;
}

int dvq_codec_record(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, const dvq_token_rule* rule, const int64_t* target,
                     uint32_t* records, int64_t rec_ld, int64_t step, int64_t* token, uint32_t* err, dvq_stream_t stream) {
    CodecParams p{};
    DVQ_REQUIRE(target && records && token && err && step >= 0 && step < rec_ld && codec_params(p, logits, dtype, B, V, ldl, rule),
                DVQ_EINVAL, "dvq_codec_record: bad arguments (V <= %d, 0 <= step < rec_ld)", CODEC_MAXV);
    DVQ_DISPATCH_DTYPE(dtype, TT, codec_record_kernel<TT><<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(p, target, records, rec_ld,
                                                                                                                  step, token, err););
    DVQ_CHECK_LAUNCH("codec_record");
    return DVQ_OK;
}

int dvq_codec_encode(const uint32_t* records, int64_t B, int64_t T, int64_t rec_ld, const int64_t* counts, const uint8_t* kinds,
                     uint32_t* words, int64_t cap, int64_t* nwords, double* bits, dvq_stream_t stream) {
    DVQ_REQUIRE(records && words && nwords && B > 0 && B < (int64_t)1 << 30 && T >= 0 && rec_ld >= T && cap >= T + 2, DVQ_EINVAL,
                "dvq_codec_encode: bad arguments (cap >= T + 2)");
    codec_encode_kernel<<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(records, rec_ld, T, counts, kinds, words, cap, nwords, bits);
    DVQ_CHECK_LAUNCH("codec_encode");
    return DVQ_OK;
}

int dvq_codec_decode_step(const void* logits, int dtype, int64_t B, int64_t V, int64_t ldl, const dvq_token_rule* rule, int64_t* state,
                          const uint32_t* words, int64_t total_words, int64_t* token, uint32_t* err, dvq_stream_t stream) {
    CodecParams p{};
    DVQ_REQUIRE(state && token && err && total_words >= 0 && (words || total_words == 0) && codec_params(p, logits, dtype, B, V, ldl, rule),
                DVQ_EINVAL, "dvq_codec_decode_step: bad arguments (V <= %d)", CODEC_MAXV);
    DVQ_DISPATCH_DTYPE(dtype, TT, codec_decode_kernel<TT><<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(p, state, words, total_words,
                                                                                                                  token, err););
    DVQ_CHECK_LAUNCH("codec_decode_step");
    return DVQ_OK;
}
