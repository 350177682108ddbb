// What the two generations of fused attention kernels share: the argument block of a call, the device helpers both kernel sets are
// written with, and the launchers attention.hip (C ABI entry points, geometry checks, the head-size-64 kernels) calls in
// attention2.hip (head sizes 128 and 256).  Not part of include/dvq_hip.h.
#pragma once
#include "dvq_common.h"

// One attention call.  The kernels of attention2.hip take exactly this block; those of attention.hip take AttnArgsCm below.
struct AttnArgs {
    const bf16_t *q, *k, *v, *o, *dout;      // [B*T][C] row-major, C = nh * head size
    bf16_t *out, *dq, *dk, *dv;
    float* lse;                              // [B][nh][T]: log-sum-exp of the scaled, masked scores (natural log)
    float* dsum;                             // [B][nh][T]: rowsum(dO * O), written by the dQ kernel, read by the dK / dV kernels
    int B, T, nh;
    int ldq;                                 // row pitch (elements) of q, k, v, dq, dk, dv: C, or 3 C when they are column blocks of one
                                             // fused [M][3 C] projection output (head size 128 only); out, o, dout always have pitch C
    float scale, inv_keep;                   // 1 / sqrt(hs), 1 / (1 - p)
    unsigned thr, rm, ra;                    // dropout: keep iff dvq_hash32(idx * rm + ra) >= thr (thr == 0: no dropout)
    unsigned long long* mask;                // optional keep-decision words, [B * nh][nqt][nkt][16] (see drop_tile): written by the
                                             // forward, read by the backward kernels instead of hashing every element again
    int causal;                              // 1: causal, head size 64 / 128;  0: full attention, one head of size 256 (AttnBlock), T % 32 == 0
    int order;                               // workgroup numbering (attention2.hip: decode_block); set by its launcher
};

// The head-size-64 kernels read the second GEMMs' A operands from channel-major copies that their entry points make first.
struct AttnArgsCm : AttnArgs {
    const bf16_t *qt, *kt, *vt, *dot;        // [B][C][T]
};

// attention2.hip.  causal: head size 128 (dropout optional); full attention: head size 256, no dropout
int dvq_attn2_fwd(const AttnArgs& a, hipStream_t stream);
int dvq_attn2_bwd(const AttnArgs& a, hipStream_t stream);

constexpr float LOG2E = 1.4426950408889634f;

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

union Frag {
    uint4 u;
    bf16x8 v;
    uint2 h[2];
};

// accumulator register r of half `half` -> row inside the 32-row tile; ccol: the part that does not depend on the lane
__device__ __forceinline__ constexpr int ccol(int r) { return (r & 3) + 8 * (r >> 2); }
__device__ __forceinline__ int crow(int r, int half) { return ccol(r) + 4 * half; }

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& a, int s) {
    Frag f;
    f.u.x = pack_bf16x2(a[8 * s + 0], a[8 * s + 1]);
    f.u.y = pack_bf16x2(a[8 * s + 2], a[8 * s + 3]);
    f.u.z = pack_bf16x2(a[8 * s + 4], a[8 * s + 5]);
    f.u.w = pack_bf16x2(a[8 * s + 6], a[8 * s + 7]);
    return f.v;
}

__device__ __forceinline__ bf16x8 ldfrag(const bf16_t* p, bool ok) {
    Frag f;
    f.u = ok ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
    return f.v;
}

// Dropout decisions of one 32 x 32 score tile as 16 lane masks.  The forward (and dQ) kernels hold the tile as lane = (query l31,
// half), register r = key crow(r, half); word r of a tile is the wave-wide ballot of "keep" for register r, i.e.
// bit (l31 + 32 half) of word r = keep(query l31, key crow(r, half)).  dQ has the same lane / register layout: word r
// IS its select mask for register r (v_cndmask with an SGPR pair: no VALU work per element besides the select).
// dK / dV hold the tile transposed (lane = key, registers = queries): lane (key kl, half h') needs keep(query crow(r', h'), kl)
// = bit crow(r', h') of the 32-bit half-word (kl >> 2 & 1) of word (kl & 3) + 4 (kl >> 3): ONE 4-byte load per lane and tile, then
// constant bit positions after a shift by 4 h'.  The hash costs 3 quarter-rate integer multiplies + 7 ALU operations per element
// (~19 issue slots against 4 for the exponential): taken once per element in the forward instead of four times per step, the three
// backward kernels drop from ~31 to ~13 VALU slots per score element (they were VALU-bound 2.5 : 1 against their MFMAs).
__device__ __forceinline__ int64_t drop_tile(int bh, int nt, int qt, int kt) { return (((int64_t)bh * nt + qt) * nt + kt) * 16; }

// [ch][row] accumulators (NM tiles of 32 channels) -> row-major [row][HS channels] bf16: lane = row, 4 consecutive channels per
// register quad (8-byte stores)
template <int NM>
__device__ __forceinline__ void store_ct(bf16_t* dst /* row base + head offset */, const f32x16 (&acc)[NM], int half, float mul) {
#pragma unroll
    for (int mt = 0; mt < NM; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 w;
            w.x = pack_bf16x2(acc[mt][4 * g + 0] * mul, acc[mt][4 * g + 1] * mul);
            w.y = pack_bf16x2(acc[mt][4 * g + 2] * mul, acc[mt][4 * g + 3] * mul);
            *reinterpret_cast<uint2*>(dst + 32 * mt + 8 * g + 4 * half) = w;
        }
}
