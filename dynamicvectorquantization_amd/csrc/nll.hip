// Teacher-forced likelihood scoring of the DQ-Transformer (gfx950, HBM-bound row work; docs/design/15-likelihood.md).  No counterpart
// in the reference: it only logs the batch means of F.cross_entropy (stackgpt.py:213-224).
//
// dvq_token_nll: one wave per row.  nll = log(sum exp(x - max)) - (x[target] - max), the sum in fp32 (the order of F.log_softmax), and the
// rank of the target among the V used columns.  A row is read ONCE: with 16-byte aligned rows of at most 2048 columns it sits in
// registers between the max, the sum and the count (token_nll_vec_kernel); any other shape takes one pass with a running maximum
// per lane (token_nll_kernel) after a single read of x[target].  Columns >= V are never loaded into a result.  Every row is written by
// exactly one lane: no atomics, no [rows, V] temporary.
// dvq_nll_segment_sums: one workgroup per (image, segment); thread t adds rows t, t + 256, ... in fp64, then a fixed tree over the
// 256 partial sums -- two launches on the same input give the same bits.
// dvq_nll_cell_sums: the same sums keyed by grid cell (docs/design/30-cell-maps.md); one owner thread per cell walks the rows in order.
#include "dvq_common.h"

#include <math.h>

namespace {

constexpr int NT = 256;

// nll / rank of one row from the wave's totals; target outside [0, V): nll = NaN, rank = V (never a top-k hit)
__device__ __forceinline__ void nll_store(float m, float s, float xt, int greater, int ties_before, bool valid, int V, int64_t r,
                                          float* __restrict__ nll, int* __restrict__ rank) {
    // the sum is fp32; its logarithm and the two differences are taken in fp64 and rounded once (one value per row: no cost)
    nll[r] = valid ? (float)(log((double)s) - ((double)xt - (double)m)) : __builtin_nanf("");
    rank[r] = valid ? greater + ties_before : V;
}

template <typename T, int NV>
__global__ __launch_bounds__(NT) void token_nll_vec_kernel(const T* __restrict__ logits, int64_t rows, int V, int ldl,
                                                           const int64_t* __restrict__ target, int64_t ignore_index,
                                                           float* __restrict__ nll, int* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    const int V8 = (V + 7) >> 3;                                     // 8-column vectors that hold a used column (V8 * 8 <= ldl)
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t tg = target[r];
        if (tg == ignore_index) {
            if (lane == 0) {
                nll[r] = 0.f;
                rank[r] = -1;
            }
            continue;
        }
        const bool valid = tg >= 0 && tg < V;
        const T* row = logits + r * ldl;
        float v[NV][8];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c8 = lane + 64 * i;
            if (c8 < V8) load8(row + c8 * 8, v[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (c8 >= V8 || c8 * 8 + j >= V) v[i][j] = -INFINITY;
                m = fmaxf(m, v[i][j]);
            }
        }
        m = wave_max(m);
        // x[target] from the lane that holds it
        const int tcol = valid ? (int)tg : 0;
        float xt = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((lane + 64 * i) * 8 + j == tcol) xt = v[i][j];
        xt = __shfl(xt, (tcol >> 3) & 63, 64);
        float s = 0.f;
        int greater = 0, ties = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = v[i][j];
                const int c = (lane + 64 * i) * 8 + j;
                s += expf(x - m);                                    // (columns >= V and -inf logits: exp(-inf) = 0)
                greater += x > xt ? 1 : 0;
                ties += (x == xt && c < tcol) ? 1 : 0;
            }
        s = wave_sum(s);
        greater = wave_sum(greater);
        ties = wave_sum(ties);
        if (lane == 0) nll_store(m, s, xt, greater, ties, valid, V, r, nll, rank);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void token_nll_kernel(const T* __restrict__ logits, int64_t rows, int V, int ldl,
                                                       const int64_t* __restrict__ target, int64_t ignore_index,
                                                       float* __restrict__ nll, int* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t tg = target[r];
        if (tg == ignore_index) {
            if (lane == 0) {
                nll[r] = 0.f;
                rank[r] = -1;
            }
            continue;
        }
        const bool valid = tg >= 0 && tg < V;
        const T* row = logits + r * ldl;
        const int tcol = valid ? (int)tg : 0;
        const float xt = ElemIO<T>::load(row + tcol);                // the one element read twice
        float m = -INFINITY, s = 0.f;                                // lane-local running maximum and sum of exp(x - m)
        int greater = 0, ties = 0;
        for (int c = lane; c < V; c += 64) {
            const float x = ElemIO<T>::load(row + c);
            greater += x > xt ? 1 : 0;
            ties += (x == xt && c < tcol) ? 1 : 0;
            if (x > m) {
                s = s * expf(m - x) + 1.f;                           // (m = -inf: s is 0 and exp(-inf) = 0)
                m = x;
            } else if (x > -INFINITY) {
                s += expf(x - m);
            }
        }
        const float mw = wave_max(m);
        s = m > -INFINITY ? s * expf(m - mw) : 0.f;                  // lanes without a finite column carry nothing
        s = wave_sum(s);
        greater = wave_sum(greater);
        ties = wave_sum(ties);
        if (lane == 0) nll_store(mw, s, xt, greater, ties, valid, V, r, nll, rank);
    }
}

__global__ __launch_bounds__(NT) void nll_segment_sums_kernel(const float* __restrict__ nll, const int* __restrict__ rank, int64_t Tp,
                                                              int64_t split, double* __restrict__ out) {
    __shared__ double red[4][NT];
    const int64_t img = blockIdx.x >> 1;
    const int seg = blockIdx.x & 1;
    const int64_t t0 = seg == 0 ? 0 : split, t1 = seg == 0 ? split : Tp;
    const int tid = threadIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};                              // nll sum, tokens, top-1 hits, top-5 hits
    for (int64_t t = t0 + tid; t < t1; t += NT) {
        const int rk = rank[img * Tp + t];
        if (rk >= 0) {
            a[0] += (double)nll[img * Tp + t];
            a[1] += 1.0;
            a[2] += rk == 0 ? 1.0 : 0.0;
            a[3] += rk < 5 ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][tid] = a[k];
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + w];
        }
        __syncthreads();
    }
    if (tid < 4) out[(img * 2 + seg) * 4 + tid] = red[tid][0];
}

// Cell of a position code under the mapping of permute_dual_back_kernel (csrc/permuter.hip): a coarse code IS its cell, a fine code is
// a raster index of the fine grid.  Anything that is no grid position (eos, pad, start tokens): ncell = "outside".
__device__ __forceinline__ int cell_of_position(int64_t pos, bool fine, int hw1, int hw2) {
    const int ncell = hw1 * hw1, fhw = hw1 * hw2;
    if (!fine) return pos >= 0 && pos < ncell ? (int)pos : ncell;
    if (pos < 0 || pos >= (int64_t)fhw * fhw) return ncell;
    const int e = (int)pos;
    return (e / fhw / hw2) * hw1 + (e % fhw) / hw2;
}

// one workgroup per (image, segment); thread t OWNS cells t, t + 256, ... (cell ncell = outside) and walks the segment's rows in row
// order, 256 rows at a time through LDS (every thread reads the same entry: a broadcast).  No atomics, one writer per output element.
__global__ __launch_bounds__(NT) void nll_cell_sums_kernel(const float* __restrict__ nll, const int* __restrict__ rank,
                                                           const int64_t* __restrict__ pos, int64_t Tp, int64_t split, int hw1, int hw2,
                                                           int stream0, int stream1, double* __restrict__ cells,
                                                           double* __restrict__ outside) {
    __shared__ int s_cell[NT];
    __shared__ float s_nll[NT];
    __shared__ int s_rank[NT];
    const int64_t img = blockIdx.x >> 1;
    const int seg = blockIdx.x & 1;
    const int stream = seg == 0 ? stream0 : stream1;
    if (stream < 0) return;
    const int64_t t0 = seg == 0 ? 0 : split, t1 = seg == 0 ? split : Tp;
    const int ncell = hw1 * hw1;
    const int tid = threadIdx.x;
    for (int cbase = 0; cbase <= ncell; cbase += NT) {
        const int mine = cbase + tid;
        double a[4] = {0.0, 0.0, 0.0, 0.0};                          // nll sum, tokens, top-1 hits, top-5 hits
        for (int64_t base = t0; base < t1; base += NT) {
            const int64_t t = base + tid;
            int c = -1;
            if (t < t1) {
                const int rk = rank[img * Tp + t];
                s_rank[tid] = rk;
                s_nll[tid] = nll[img * Tp + t];
                if (rk >= 0) c = cell_of_position(pos[img * Tp + t], seg == 1, hw1, hw2);
            }
            s_cell[tid] = c;                                         // -1: ignored row or past the segment
            __syncthreads();
            const int n = (int)(t1 - base < NT ? t1 - base : NT);
            for (int k = 0; k < n; ++k) {
                if (s_cell[k] == mine) {
                    const int rk = s_rank[k];
                    a[0] += (double)s_nll[k];
                    a[1] += 1.0;
                    a[2] += rk == 0 ? 1.0 : 0.0;
                    a[3] += rk < 5 ? 1.0 : 0.0;
                }
            }
            __syncthreads();
        }
        if (mine <= ncell) {
            double* o = mine < ncell ? cells + ((img * 4 + stream) * ncell + mine) * 4 : outside + (img * 4 + stream) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = a[k];
        }
    }
}

}  // namespace

int dvq_nll_cell_sums(const float* nll, const int32_t* rank, const int64_t* pos, int64_t B, int64_t Tp, int64_t split, int hw1, int hw2,
                      int stream0, int stream1, double* cells, double* outside, dvq_stream_t stream) {
    DVQ_REQUIRE(nll && rank && pos && cells && outside && B > 0 && B < (int64_t)1 << 30 && Tp > 0 && split >= 0 && split <= Tp, DVQ_EINVAL,
                "dvq_nll_cell_sums: bad arguments");
    DVQ_REQUIRE(hw1 > 0 && hw2 > 0 && (int64_t)hw1 * hw2 <= 4096 && stream0 >= -1 && stream0 < 4 && stream1 >= -1 && stream1 < 4 &&
                    (stream0 != stream1 || stream0 < 0),
                DVQ_ESHAPE, "dvq_nll_cell_sums: hw1=%d hw2=%d streams %d / %d", hw1, hw2, stream0, stream1);
    nll_cell_sums_kernel<<<dim3((unsigned)(2 * B)), dim3(NT), 0, (hipStream_t)stream>>>(nll, rank, pos, Tp, split, hw1, hw2, stream0, stream1,
                                                                                       cells, outside);
    DVQ_CHECK_LAUNCH("nll_cell_sums");
    return DVQ_OK;
}

int dvq_token_nll(const void* logits, int dtype, int64_t rows, int64_t V, int64_t ldl, const int64_t* target, int64_t ignore_index,
                  float* nll, int32_t* rank, dvq_stream_t stream) {
    DVQ_REQUIRE(logits && target && nll && rank && rows > 0 && V > 0 && ldl >= V && ldl < (int64_t)1 << 31 &&
                    (dtype == DVQ_F32 || dtype == DVQ_BF16),
                DVQ_EINVAL, "dvq_token_nll: bad arguments");
    int64_t b = cdiv64(rows, 4);
    const dim3 grid((unsigned)(b > 65536 ? 65536 : b)), block(NT);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = ldl % 8 == 0 && V <= 64 * 8 * 4 && ((uintptr_t)logits & 15) == 0;
    if (vec && V <= 64 * 8 * 2) {
        DVQ_DISPATCH_DTYPE(dtype, T, token_nll_vec_kernel<T, 2><<<grid, block, 0, st>>>((const T*)logits, rows, (int)V, (int)ldl, target,
                                                                                       ignore_index, nll, rank););
    } else if (vec) {
        DVQ_DISPATCH_DTYPE(dtype, T, token_nll_vec_kernel<T, 4><<<grid, block, 0, st>>>((const T*)logits, rows, (int)V, (int)ldl, target,
                                                                                       ignore_index, nll, rank););
    } else {
        DVQ_DISPATCH_DTYPE(dtype, T, token_nll_kernel<T><<<grid, block, 0, st>>>((const T*)logits, rows, (int)V, (int)ldl, target,
                                                                                ignore_index, nll, rank););
    }
    DVQ_CHECK_LAUNCH("token_nll");
    return DVQ_OK;
}

int dvq_nll_segment_sums(const float* nll, const int32_t* rank, int64_t B, int64_t Tp, int64_t split, double* out, dvq_stream_t stream) {
    DVQ_REQUIRE(nll && rank && out && B > 0 && B < (int64_t)1 << 30 && Tp > 0 && split >= 0 && split <= Tp, DVQ_EINVAL,
                "dvq_nll_segment_sums: bad arguments");
    nll_segment_sums_kernel<<<dim3((unsigned)(2 * B)), dim3(NT), 0, (hipStream_t)stream>>>(nll, rank, Tp, split, out);
    DVQ_CHECK_LAUNCH("nll_segment_sums");
    return DVQ_OK;
}
