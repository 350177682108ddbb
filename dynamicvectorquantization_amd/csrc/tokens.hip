// Token shards (docs/design/16-token-shards.md): the stored form of a dual-grain code map and its way back to the stage-2 streams.
//   dvq_tokens_pack    encode()'s int64 code map + grain map -> u16 codes, a grain bitmap (bit c % 32 of word c / 32 = cell c is fine,
//                      built from wave ballots), the number of fine cells and a count of out-of-range inputs per image
//   dvq_tokens_unpack  u16 codes + bitmap -> the four EOS-terminated, PAD-filled int64 rows of DualGrainSeperatePermuter.forward
//                      (csrc/permuter.hip), bit for bit, at row lengths given by the HOST (it has the bitmap: no device read-back)
// Unpack needs no scan over cells or pixels: with pre[c] = fine cells before cell c (popcount of whole bitmap words + one masked word)
// every output slot has a closed form.  q = hw2 * hw2:
//   coarse cell c                        -> slot c - pre[c]
//   fine pixel (y, x) of cell c, region-first -> pre[c] * q + (y % hw2) * hw2 + x % hw2
//   row-first, cy = y / hw2, r0 = pre[cy * hw1], nrow = fine cells of cell-row cy
//                                        -> r0 * q + (y % hw2) * hw2 * nrow + (pre[c] - r0) * hw2 + x % hw2
// One workgroup per image; the word prefixes of up to 1024 cells (32 words) come from one wave's shuffle scan and sit in LDS behind one
// barrier.  Integer work, a few KB per image: launch-bound.
#include "dvq_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_WORDS = 32;      // 1024 cells

struct PackParams {
    const int64_t* idx;      // [B, npix]
    const int64_t* grain;    // [B, ncell]
    int ncell, npix, words;
    int64_t klim;            // min(codebook_size, 65536)
    uint16_t* codes;         // [B, npix]
    uint32_t* bits;          // [B, words]
    int* n_fine;             // [B]
    int* bad;                // [B]
};

__global__ __launch_bounds__(NT) void tokens_pack_kernel(PackParams p) {
    __shared__ int s_fine, s_bad;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63;
    if (t == 0) {
        s_fine = 0;
        s_bad = 0;
    }
    __syncthreads();
    const int64_t* idx = p.idx + (int64_t)b * p.npix;
    const int64_t* gr = p.grain + (int64_t)b * p.ncell;
    uint16_t* codes = p.codes + (int64_t)b * p.npix;
    uint32_t* bits = p.bits + (int64_t)b * p.words;
    int bad = 0;
    for (int e = t; e < p.npix; e += NT) {
        int64_t v = idx[e];
        if (v < 0 || v >= p.klim) {
            ++bad;
            v = v < 0 ? 0 : p.klim - 1;
        }
        codes[e] = (uint16_t)v;
    }
    // the trip count is uniform over the workgroup: every ballot sees whole waves; cells past the grid vote 0
    for (int base = 0; base < p.ncell; base += NT) {
        const int c = base + t;
        const int64_t g = c < p.ncell ? gr[c] : 0;
        bad += g != 0 && g != 1;
        const unsigned long long vote = __ballot(g == 1);
        if (lane == 0) {
            const int w = (c >> 5);                       // c is a multiple of 64 here
            if (w < p.words) bits[w] = (uint32_t)vote;
            if (w + 1 < p.words) bits[w + 1] = (uint32_t)(vote >> 32);
            if (vote) atomicAdd(&s_fine, __popcll(vote));
        }
    }
    bad = wave_sum(bad);
    if (lane == 0 && bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    if (t == 0) {
        p.n_fine[b] = s_fine;
        p.bad[b] = s_bad;
    }
}

struct UnpackParams {
    const uint16_t* codes;   // [B, npix]
    const uint32_t* bits;    // [B, words]
    int hw1, hw2, order, words;
    int Lc, Lf;
    int64_t content_pad, content_eos, cpos_pad, cpos_eos, fpos_pad, fpos_eos;
    int64_t *cc, *cp, *fc, *fp;   // [B, Lc], [B, Lc], [B, Lf], [B, Lf]
};

__global__ __launch_bounds__(NT) void tokens_unpack_kernel(UnpackParams p) {
    __shared__ uint32_t s_word[MAX_WORDS + 1];
    __shared__ int s_pre[MAX_WORDS + 1];             // fine cells before word w; entries words .. MAX_WORDS hold the total
    const int b = blockIdx.x, t = threadIdx.x;
    const int ncell = p.hw1 * p.hw1, fhw = p.hw1 * p.hw2, npix = fhw * fhw, q = p.hw2 * p.hw2;
    if (t < 64) {
        uint32_t w = t < p.words ? p.bits[(int64_t)b * p.words + t] : 0u;
        if (t == (ncell >> 5)) w &= (1u << (ncell & 31)) - 1u;      // bits past the grid never count (ncell % 32 == 0: t == words)
        const int n = __popc(w);
        int incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (t >= o) incl += up;
        }
        if (t <= MAX_WORDS) {
            s_word[t] = w;
            s_pre[t] = incl - n;
        }
    }
    __syncthreads();
    auto pre = [&](int c) { return s_pre[c >> 5] + __popc(s_word[c >> 5] & ((1u << (c & 31)) - 1u)); };      // c in [0, ncell]
    auto fine = [&](int c) { return (s_word[c >> 5] >> (c & 31)) & 1u; };
    const int nfine = s_pre[MAX_WORDS];
    const int ncoarse = ncell - nfine, nf = nfine * q;
    const uint16_t* codes = p.codes + (int64_t)b * npix;
    int64_t* cc = p.cc + (int64_t)b * p.Lc;
    int64_t* cp = p.cp + (int64_t)b * p.Lc;
    int64_t* fc = p.fc + (int64_t)b * p.Lf;
    int64_t* fp = p.fp + (int64_t)b * p.Lf;
    for (int c = t; c < ncell; c += NT) {
        if (fine(c)) continue;
        const int slot = c - pre(c);
        if (slot < p.Lc) {
            const int h1 = c / p.hw1, w1 = c - h1 * p.hw1;
            cc[slot] = codes[(h1 * p.hw2) * fhw + w1 * p.hw2];
            cp[slot] = c;
        }
    }
    for (int e = t; e < npix; e += NT) {
        const int y = e / fhw, x = e - y * fhw;
        const int cy = y / p.hw2, cx = x / p.hw2;
        const int c = cy * p.hw1 + cx;
        if (!fine(c)) continue;
        const int y2 = y - cy * p.hw2, x2 = x - cx * p.hw2;
        int slot;
        if (p.order == 0) {
            slot = pre(c) * q + y2 * p.hw2 + x2;
        } else {
            const int r0 = pre(cy * p.hw1), nrow = pre((cy + 1) * p.hw1) - r0;
            slot = r0 * q + y2 * p.hw2 * nrow + (pre(c) - r0) * p.hw2 + x2;
        }
        if (slot < p.Lf) {
            fc[slot] = codes[e];
            fp[slot] = e;
        }
    }
    for (int e = ncoarse + t; e < p.Lc; e += NT) {
        cc[e] = e == ncoarse ? p.content_eos : p.content_pad;
        cp[e] = e == ncoarse ? p.cpos_eos : p.cpos_pad;
    }
    for (int e = nf + t; e < p.Lf; e += NT) {
        fc[e] = e == nf ? p.content_eos : p.content_pad;
        fp[e] = e == nf ? p.fpos_eos : p.fpos_pad;
    }
}

}  // namespace

extern "C" {

int dvq_tokens_pack(const int64_t* indices, const int64_t* grain, int64_t B, int hw1, int hw2, int64_t codebook_size, uint16_t* codes,
                    uint32_t* grain_bits, int32_t* n_fine_cells, int32_t* bad, dvq_stream_t stream) {
    DVQ_REQUIRE(indices && grain && codes && grain_bits && n_fine_cells && bad, DVQ_EINVAL, "dvq_tokens_pack: null pointer");
    DVQ_REQUIRE(B > 0 && B < (1 << 30) && hw1 > 0 && hw2 > 0 && hw1 * hw2 <= 256 && codebook_size > 0, DVQ_ESHAPE,
                "dvq_tokens_pack: bad geometry (B %lld, hw1 %d, hw2 %d, codebook_size %lld)", (long long)B, hw1, hw2,
                (long long)codebook_size);
    PackParams p{};
    p.idx = indices; p.grain = grain;
    p.ncell = hw1 * hw1; p.npix = p.ncell * hw2 * hw2; p.words = (p.ncell + 31) / 32;
    p.klim = codebook_size < 65536 ? codebook_size : 65536;
    p.codes = codes; p.bits = grain_bits; p.n_fine = n_fine_cells; p.bad = bad;
    tokens_pack_kernel<<<dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream>>>(p);
    DVQ_CHECK_LAUNCH("tokens_pack");
    return DVQ_OK;
}

int dvq_tokens_unpack(const uint16_t* codes, const uint32_t* grain_bits, int64_t B, int hw1, int hw2, int order, int64_t content_pad,
                      int64_t content_eos, int64_t cpos_pad, int64_t cpos_eos, int64_t fpos_pad, int64_t fpos_eos, int64_t Lc, int64_t Lf,
                      int64_t* coarse_content, int64_t* coarse_position, int64_t* fine_content, int64_t* fine_position,
                      dvq_stream_t stream) {
    DVQ_REQUIRE(codes && grain_bits && coarse_content && coarse_position && fine_content && fine_position, DVQ_EINVAL,
                "dvq_tokens_unpack: null pointer");
    DVQ_REQUIRE(B > 0 && B < (1 << 30) && hw1 > 0 && hw2 > 0 && hw1 * hw1 <= 32 * MAX_WORDS && hw1 * hw2 <= 256 &&
                    (order == 0 || order == 1) && Lc > 0 && Lf > 0 && Lc < (1 << 30) && Lf < (1 << 30),
                DVQ_ESHAPE, "dvq_tokens_unpack: bad geometry (hw1 %d: at most 1024 cells; hw2 %d, order %d, Lc %lld, Lf %lld)", hw1, hw2,
                order, (long long)Lc, (long long)Lf);
    UnpackParams p{};
    p.codes = codes; p.bits = grain_bits; p.hw1 = hw1; p.hw2 = hw2; p.order = order; p.words = (hw1 * hw1 + 31) / 32;
    p.Lc = (int)Lc; p.Lf = (int)Lf;
    p.content_pad = content_pad; p.content_eos = content_eos; p.cpos_pad = cpos_pad; p.cpos_eos = cpos_eos;
    p.fpos_pad = fpos_pad; p.fpos_eos = fpos_eos;
    p.cc = coarse_content; p.cp = coarse_position; p.fc = fine_content; p.fp = fine_position;
    tokens_unpack_kernel<<<dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream>>>(p);
    DVQ_CHECK_LAUNCH("tokens_unpack");
    return DVQ_OK;
}

}  // extern "C"
