// The token rule of include/dvq_hip.h (dvq_token_rule) as the sampler (transformer.hip) and the token codec (codec.hip) apply it: the
// ONLY copy of its argument check, its normalisation, its per-row flags and its per-column predicate.  A bitstream decodes only
// while the codec's tables use exactly the rule the sampler draws under, so neither file restates any of it.
#pragma once
#include "dvq_common.h"

struct TokenRule {                  // the normalised rule a kernel carries in its parameter block (by value)
    const int64_t* forbid_idx;
    int64_t forbid_ld;
    int n_forbid;                   // 0 without a list
    int forbid_from;                // in [0, V]
    int codes[4];
    int keep_code, late_forbid_code, pad_code;
    const float* finished;
};

// host: check `rule` for B rows of V columns (0 < B < 2^30, 0 < V <= DVQ_TOKEN_RULE_MAXV) and normalise it into `r`; false on a bad
// rule or range (r is then unspecified)
inline bool token_rule_fill(TokenRule& r, const dvq_token_rule* rule, int64_t B, int64_t V) {
    constexpr int64_t LIM = (int64_t)1 << 30;
    if (!(rule && B > 0 && B < LIM && V > 0 && V <= DVQ_TOKEN_RULE_MAXV && rule->pad_code >= 0 && rule->pad_code < V &&
          (rule->forbid_idx == nullptr || (rule->n_forbid >= 0 && rule->n_forbid < LIM && rule->forbid_ld >= rule->n_forbid))))
        return false;
    r.forbid_idx = rule->forbid_idx; r.forbid_ld = rule->forbid_ld; r.n_forbid = rule->forbid_idx ? (int)rule->n_forbid : 0;
    r.forbid_from = (int)(rule->forbid_from < 0 || rule->forbid_from > V ? V : rule->forbid_from);
    for (int i = 0; i < 4; ++i) r.codes[i] = (int)rule->forbid_codes4[i];
    r.keep_code = (int)rule->keep_code; r.late_forbid_code = (int)rule->late_forbid_code; r.pad_code = (int)rule->pad_code;
    r.finished = rule->finished;
    return true;
}

__device__ __forceinline__ bool token_rule_finished(const TokenRule& r, int row) { return r.finished != nullptr && r.finished[row] != 0.f; }

// flag[0 .. V) = 1 on the columns listed for a live `row`, 0 elsewhere (cleared up to nflag >= V: the sampler clears its whole sort
// size, as it always has); every thread of the workgroup (nth threads, this one tid) calls it, and flag[] is ready for all on return
__device__ __forceinline__ void token_rule_mark(const TokenRule& r, bool fin, int row, int V, unsigned char* flag, int nflag, int tid,
                                                int nth) {
    for (int c = tid; c < nflag; c += nth) flag[c] = 0;
    __syncthreads();
    if (!fin && r.forbid_idx != nullptr)
        for (int j = tid; j < r.n_forbid; j += nth) {
            const int64_t c = r.forbid_idx[(int64_t)row * r.forbid_ld + j];
            if (c >= 0 && c < V) flag[c] = 1;
        }
    __syncthreads();
}

// is column c (0 <= c < V) of a row masked?  (flag: token_rule_mark's)
__device__ __forceinline__ bool token_rule_masked(const TokenRule& r, bool fin, const unsigned char* flag, int c) {
    if (fin) return c != r.pad_code;
    bool masked = flag[c] != 0 || c >= r.forbid_from || c == r.codes[0] || c == r.codes[1] || c == r.codes[2] || c == r.codes[3];
    if (c == r.keep_code) masked = false;
    if (c == r.late_forbid_code) masked = true;
    return masked;
}
