// Per-segment statistics of a flat fp32 buffer (docs/design/24-norm-tracking.md): sum of squares, abs-max and the count of Inf / NaN
// elements of every parameter's slice of an optimizer's flat gradient / parameter buffer, or of the difference of two buffers.
//
// The ordered two-stage form of grad_sqnorm (misc.hip), segmented.  A plan built once on the host cuts every segment into chunks of
// SEG_CHUNK elements (the last one shorter); a chunk never crosses a segment boundary.
//   Stage 1: workgroup c owns chunk c and stores ONE partial {fp64 sumsq, fp32 absmax, int32 nonfinite} with plain stores.  Element i of
//            a chunk goes to thread (i / 4) % 256, accumulator i % 4 -- with 16-byte loads where the chunk starts on a 16-byte
//            boundary in every operand, with 4-byte loads elsewhere: the assignment is a function of the chunk alone.
//   Stage 2: one wave per segment; lane l adds the segment's partials l, l + 64, ... in increasing index, the 64 lanes meet in
//            wave_sum's fixed tree, lane 0 writes the segment's row of the state block (and, sticky, its running counters).
// No atomics; the number of partials and the order of every addition depend on the segment table alone, never on the grid, the CU
// count or the arrival order of workgroups: equal inputs give bit-equal state on every launch and every device.
#include "dvq_common.h"

namespace {

constexpr int64_t SEG_CHUNK = 32768;      // == SQNORM_CHUNK of misc.hip (kernels.GRAD_SQNORM_CHUNK)

struct SegChunk {
    int64_t start;      // element offset in the flat buffer
    int32_t seg;
    int32_t len;        // 1 .. SEG_CHUNK
};

struct SegPartial {
    double sumsq;
    float absmax;
    int32_t nonfinite;
};

struct PlanHeader {
    int64_t n, S, nchunks, chunk;
};
// plan = PlanHeader | int64 offsets[S + 1] | int64 chunk0[S + 1] (first chunk of each segment, chunk0[S] = nchunks) | SegChunk[nchunks]

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

struct Acc {
    double sq;
    float mx;
    int bad;
};

// one element: v = a (or a - b, exact in fp64); an Inf / NaN operand counts and contributes nothing else
template <bool DIFF>
__device__ __forceinline__ void seg_elem(Acc& acc, float x, float y) {
    const bool fin = DIFF ? (finite_f32(x) && finite_f32(y)) : finite_f32(x);
    const double v = fin ? (DIFF ? (double)x - (double)y : (double)x) : 0.0;
    acc.sq += v * v;
    acc.mx = fmaxf(acc.mx, (float)fabs(v));
    acc.bad += fin ? 0 : 1;
}

template <bool DIFF>
__global__ __launch_bounds__(256) void segment_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              const SegChunk* __restrict__ chunks,
                                                              SegPartial* __restrict__ partial, const int* __restrict__ armed) {
    if (armed != nullptr && *armed == 0) return;
    __shared__ double psq[4];
    __shared__ float pmx[4];
    __shared__ int pbad[4];
    const SegChunk ck = chunks[blockIdx.x];
    const int len = ck.len;
    const float* ac = a + ck.start;
    const float* bc = DIFF ? b + ck.start : nullptr;
    const int nvec = len >> 2;
    Acc a0{0.0, 0.f, 0}, a1{0.0, 0.f, 0}, a2{0.0, 0.f, 0}, a3{0.0, 0.f, 0};
    const bool vec = (((uintptr_t)ac | (DIFF ? (uintptr_t)bc : 0)) & 15) == 0;      // workgroup-uniform
    if (vec) {
#pragma unroll 4
        for (int q = threadIdx.x; q < nvec; q += 256) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(ac + 4 * q);
            f32x4 y = {0.f, 0.f, 0.f, 0.f};
            if (DIFF) y = *reinterpret_cast<const f32x4*>(bc + 4 * q);
            seg_elem<DIFF>(a0, x[0], y[0]);
            seg_elem<DIFF>(a1, x[1], y[1]);
            seg_elem<DIFF>(a2, x[2], y[2]);
            seg_elem<DIFF>(a3, x[3], y[3]);
        }
    } else {
#pragma unroll 4
        for (int q = threadIdx.x; q < nvec; q += 256) {
            const float x0 = ac[4 * q], x1 = ac[4 * q + 1], x2 = ac[4 * q + 2], x3 = ac[4 * q + 3];
            float y0 = 0.f, y1 = 0.f, y2 = 0.f, y3 = 0.f;
            if (DIFF) {
                y0 = bc[4 * q]; y1 = bc[4 * q + 1]; y2 = bc[4 * q + 2]; y3 = bc[4 * q + 3];
            }
            seg_elem<DIFF>(a0, x0, y0);
            seg_elem<DIFF>(a1, x1, y1);
            seg_elem<DIFF>(a2, x2, y2);
            seg_elem<DIFF>(a3, x3, y3);
        }
    }
    const int tail = 4 * nvec + (int)threadIdx.x;                          // len % 4 leftover elements: threads 0..2
    if (threadIdx.x < 3 && tail < len) seg_elem<DIFF>(a0, ac[tail], DIFF ? bc[tail] : 0.f);
    const double sq = wave_sum((a0.sq + a1.sq) + (a2.sq + a3.sq));
    const float mx = wave_max(fmaxf(fmaxf(a0.mx, a1.mx), fmaxf(a2.mx, a3.mx)));
    const int bad = wave_sum((a0.bad + a1.bad) + (a2.bad + a3.bad));
    if ((threadIdx.x & 63) == 0) {
        psq[threadIdx.x >> 6] = sq;
        pmx[threadIdx.x >> 6] = mx;
        pbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        SegPartial out;
        out.sumsq = (psq[0] + psq[1]) + (psq[2] + psq[3]);
        out.absmax = fmaxf(fmaxf(pmx[0], pmx[1]), fmaxf(pmx[2], pmx[3]));
        out.nonfinite = (pbad[0] + pbad[1]) + (pbad[2] + pbad[3]);
        partial[blockIdx.x] = out;
    }
}

// state = double sumsq[S] | int64 nonfinite[S] | int64 nonfinite_total[S] | int64 first_bad_call[S] | int64 calls[S] | float absmax[S]
// (calls: the block's launch counter, kept once per segment so that every owner reads and advances its own copy -- no owner waits
// for another; all S copies are equal between launches)
__global__ __launch_bounds__(256) void segment_final_kernel(const SegPartial* __restrict__ partial, const int64_t* __restrict__ chunk0,
                                                            int64_t S, void* __restrict__ state, int sticky,
                                                            const int* __restrict__ armed) {
    if (armed != nullptr && *armed == 0) return;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;                                                     // whole waves leave: the shuffles below see full waves
    const int lane = threadIdx.x & 63;
    const int64_t c0 = chunk0[s], c1 = chunk0[s + 1];
    double sq = 0.0;
    float mx = 0.f;
    int64_t bad = 0;
    for (int64_t c = c0 + lane; c < c1; c += 64) {
        const SegPartial p = partial[c];
        sq += p.sumsq;
        mx = fmaxf(mx, p.absmax);
        bad += p.nonfinite;
    }
    sq = wave_sum(sq);
    mx = wave_max(mx);
    bad = wave_sum(bad);
    if (lane != 0) return;
    double* sumsq = reinterpret_cast<double*>(state);
    int64_t* nonfinite = reinterpret_cast<int64_t*>(state) + S;
    int64_t* total = nonfinite + S;
    int64_t* first_bad = total + S;
    int64_t* calls = first_bad + S;
    float* absmax = reinterpret_cast<float*>(calls + S);
    sumsq[s] = sq;
    nonfinite[s] = bad;
    absmax[s] = mx;
    if (sticky) {
        const int64_t call = calls[s];
        if (bad != 0) {
            total[s] += bad;
            if (first_bad[s] < 0) first_bad[s] = call;
        }
        calls[s] = call + 1;
    }
}

// VEC: 16-byte accesses, two per thread in flight, the n % 4 tail by threads 0..2 of block 0; !VEC: 4-byte accesses
template <bool VEC>
__global__ __launch_bounds__(256) void copy_f32_armed_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n,
                                                             const int* __restrict__ armed) {
    if (armed != nullptr && *armed == 0) return;
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int64_t nvec = n >> 2;
        f32x4* dv = reinterpret_cast<f32x4*>(dst);
        const f32x4* sv = reinterpret_cast<const f32x4*>(src);
        for (; i + stride < nvec; i += 2 * stride) {
            const f32x4 s0 = sv[i], s1 = sv[i + stride];
            dv[i] = s0;
            dv[i + stride] = s1;
        }
        if (i < nvec) dv[i] = sv[i];
        const int64_t t = 4 * nvec + threadIdx.x;
        if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) dst[t] = src[t];
    } else {
        for (; i < n; i += stride) dst[i] = src[i];
    }
}

inline unsigned copy_blocks(int64_t work, int64_t per_block) {
    int64_t b = cdiv64(work, per_block);
    if (b < 1) b = 1;
    if (b > 4096) b = 4096;
    return (unsigned)b;
}

// ascending offsets from 0 to n, every length >= 1 -> number of chunks; -1 otherwise
int64_t plan_chunks(const int64_t* off, int64_t S, int64_t n) {
    if (off == nullptr || S < 1 || S > 0x7fffffff || n < S || off[0] != 0 || off[S] != n) return -1;
    int64_t chunks = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t len = off[s + 1] - off[s];
        if (len < 1 || off[s + 1] > n) return -1;
        chunks += cdiv64(len, SEG_CHUNK);
    }
    return chunks <= 0x7fffffff ? chunks : -1;
}

size_t plan_bytes(int64_t S, int64_t nchunks) {
    return sizeof(PlanHeader) + 2 * (size_t)(S + 1) * sizeof(int64_t) + (size_t)nchunks * sizeof(SegChunk);
}

}  // namespace

extern "C" {

size_t dvq_segment_stats_workspace_bytes(int64_t n, int64_t S) {
    // a segment's last chunk may be short: at most n / chunk full chunks plus one tail per segment
    return (n > 0 && S > 0 && S <= n) ? (size_t)(n / SEG_CHUNK + S) * sizeof(SegPartial) : 0;
}

size_t dvq_segment_stats_state_bytes(int64_t S) { return S > 0 ? (size_t)S * 40 + (((size_t)S * 4 + 7) & ~(size_t)7) : 0; }

size_t dvq_segment_plan_bytes(const int64_t* offsets, int64_t S, int64_t n) {
    const int64_t chunks = plan_chunks(offsets, S, n);
    return chunks < 0 ? 0 : plan_bytes(S, chunks);
}

int dvq_segment_plan_build(const int64_t* offsets, int64_t S, int64_t n, void* plan_host, size_t plan_host_bytes) {
    const int64_t chunks = plan_chunks(offsets, S, n);
    DVQ_REQUIRE(chunks >= 0, DVQ_ESHAPE, "dvq_segment_plan_build: offsets must rise from 0 to n in steps >= 1 (S = %lld, n = %lld)",
                (long long)S, (long long)n);
    DVQ_REQUIRE(plan_host != nullptr && plan_host_bytes >= plan_bytes(S, chunks) && ((uintptr_t)plan_host & 7) == 0, DVQ_EINVAL,
                "dvq_segment_plan_build: plan buffer of %zu bytes, %zu needed, 8-byte aligned", plan_host_bytes, plan_bytes(S, chunks));
    PlanHeader* h = reinterpret_cast<PlanHeader*>(plan_host);
    *h = PlanHeader{n, S, chunks, SEG_CHUNK};
    int64_t* off = reinterpret_cast<int64_t*>(h + 1);
    int64_t* chunk0 = off + (S + 1);
    SegChunk* ck = reinterpret_cast<SegChunk*>(chunk0 + (S + 1));
    int64_t c = 0;
    for (int64_t s = 0; s < S; ++s) {
        off[s] = offsets[s];
        chunk0[s] = c;
        for (int64_t at = offsets[s]; at < offsets[s + 1]; at += SEG_CHUNK) {
            const int64_t rest = offsets[s + 1] - at;
            ck[c++] = SegChunk{at, (int32_t)s, (int32_t)(rest < SEG_CHUNK ? rest : SEG_CHUNK)};
        }
    }
    off[S] = n;
    chunk0[S] = c;
    return DVQ_OK;
}

int dvq_segment_stats(const float* a, const float* b, int64_t n, const int64_t* offsets, int64_t S, const void* plan_dev,
                      size_t plan_bytes_given, void* workspace, size_t workspace_bytes, void* state, int sticky, const int* armed,
                      dvq_stream_t stream) {
    DVQ_REQUIRE(a && offsets && plan_dev && workspace && state && n > 0, DVQ_EINVAL, "dvq_segment_stats: bad arguments");
    const int64_t chunks = plan_chunks(offsets, S, n);
    DVQ_REQUIRE(chunks >= 0, DVQ_ESHAPE, "dvq_segment_stats: offsets must rise from 0 to n in steps >= 1 (S = %lld, n = %lld)",
                (long long)S, (long long)n);
    DVQ_REQUIRE(plan_bytes_given == plan_bytes(S, chunks), DVQ_ESHAPE,
                "dvq_segment_stats: a plan of %zu bytes does not belong to these offsets (%zu)", plan_bytes_given, plan_bytes(S, chunks));
    DVQ_REQUIRE(workspace_bytes >= (size_t)chunks * sizeof(SegPartial), DVQ_EWORKSPACE,
                "dvq_segment_stats: workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)chunks * sizeof(SegPartial));
    DVQ_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)armed) & 3) == 0 &&
                    (((uintptr_t)plan_dev | (uintptr_t)workspace | (uintptr_t)state) & 7) == 0,
                DVQ_EINVAL, "dvq_segment_stats: a, b, armed must be 4-byte, plan, workspace and state 8-byte aligned");
    const char* plan = reinterpret_cast<const char*>(plan_dev);
    const int64_t* chunk0 = reinterpret_cast<const int64_t*>(plan + sizeof(PlanHeader)) + (S + 1);
    const SegChunk* ck = reinterpret_cast<const SegChunk*>(chunk0 + (S + 1));
    SegPartial* part = reinterpret_cast<SegPartial*>(workspace);
    if (b != nullptr)
        segment_partial_kernel<true><<<dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream>>>(a, b, ck, part, armed);
    else
        segment_partial_kernel<false><<<dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream>>>(a, nullptr, ck, part, armed);
    DVQ_CHECK_LAUNCH("segment_partial");
    segment_final_kernel<<<dim3((unsigned)cdiv64(S, 4)), dim3(256), 0, (hipStream_t)stream>>>(part, chunk0, S, state, sticky ? 1 : 0, armed);
    DVQ_CHECK_LAUNCH("segment_final");
    return DVQ_OK;
}

int dvq_copy_f32_armed(float* dst, const float* src, int64_t n, const int* armed, dvq_stream_t stream) {
    DVQ_REQUIRE(dst && src && n > 0, DVQ_EINVAL, "dvq_copy_f32_armed: bad arguments");
    DVQ_REQUIRE((((uintptr_t)dst | (uintptr_t)src | (uintptr_t)armed) & 3) == 0, DVQ_EINVAL,
                "dvq_copy_f32_armed: dst, src and armed must be 4-byte aligned");
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0)
        copy_f32_armed_kernel<true><<<dim3(copy_blocks(n >> 2, 512)), dim3(256), 0, (hipStream_t)stream>>>(dst, src, n, armed);
    else
        copy_f32_armed_kernel<false><<<dim3(copy_blocks(n, 1024)), dim3(256), 0, (hipStream_t)stream>>>(dst, src, n, armed);
    DVQ_CHECK_LAUNCH("copy_f32_armed");
    return DVQ_OK;
}

}  // extern "C"
