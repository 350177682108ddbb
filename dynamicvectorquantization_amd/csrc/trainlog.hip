// Training metric logs (docs/design/22-metrics-logging.md): the device side of metrics.MetricsLogger.
//
// dvq_scalar_push gathers the scalars a model logged in one step -- device scalars of several types plus host numbers -- into one
// caller-owned state block: the last value, an fp64 running sum, the count of finite values and the count of non-finite ones, per column.
// The scalars are described BY VALUE in the launch arguments ((address, type code) pairs, 576 bytes): a recorded step keeps its own
// copy of the record in the kernel node, no pointer table lives in device memory and no copy node enters the recording.
// dvq_codebook_health turns the per-code counts of a quantiser's step into perplexity / active codes / tokens and adds the counts to an
// fp64 running total.
//
// Both are single-workgroup kernels with one owner thread per output element: no atomics, the order of every addition is fixed by the
// arguments, equal inputs give bit-equal state.
#include <math.h>

#include "dvq_common.h"

namespace {

constexpr int PUSH_MAX = DVQ_SCALAR_PUSH_MAX;           // scalars per launch
constexpr int PUSH_COLUMNS_MAX = DVQ_SCALAR_COLUMNS_MAX;

// state block of `columns` columns: double sum[columns] | int64 cnt[columns] | int64 bad[columns] | float last[columns]
__global__ __launch_bounds__(PUSH_MAX) void scalar_push_kernel(const dvq_scalar_record rec, int count, int col0, int columns,
                                                               void* __restrict__ state) {
    const int t = threadIdx.x;
    if (t >= count || rec.code[t] == DVQ_SCALAR_SKIP) return;
    const uint64_t a = rec.addr[t];
    double v;
    float last;
    bool finite = true;
    switch (rec.code[t]) {
        case DVQ_SCALAR_F32:
            last = *reinterpret_cast<const float*>(a), v = (double)last, finite = isfinite(last);
            break;
        case DVQ_SCALAR_BF16:
            last = bf16_to_f32(*reinterpret_cast<const bf16_t*>(a)), v = (double)last, finite = isfinite(last);
            break;
        case DVQ_SCALAR_F64:
            v = *reinterpret_cast<const double*>(a), last = (float)v, finite = isfinite(v);
            break;
        case DVQ_SCALAR_I32: {
            const int32_t i = *reinterpret_cast<const int32_t*>(a);
            v = (double)i, last = (float)i;
            break;
        }
        case DVQ_SCALAR_I64: {
            const int64_t i = *reinterpret_cast<const int64_t*>(a);
            v = (double)i, last = (float)i;
            break;
        }
        default:                                   // DVQ_SCALAR_IMM: the value itself, an fp64 bit pattern in the address slot
            v = __longlong_as_double((long long)a), last = (float)v, finite = isfinite(v);
            break;
    }
    const int c = col0 + t;
    double* sum = reinterpret_cast<double*>(state);
    int64_t* cnt = reinterpret_cast<int64_t*>(sum + columns);
    int64_t* bad = cnt + columns;
    float* lastp = reinterpret_cast<float*>(bad + columns);
    lastp[c] = last;
    if (finite) {
        sum[c] += v;
        cnt[c] += 1;
    } else {
        bad[c] += 1;
    }
}

constexpr int HEALTH_NT = 256;

// fixed tree over the workgroup's partials: the result depends on (K, counts) alone
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                               // the previous use of `red` has been read
    red[t] = v;
    __syncthreads();
    for (int s = HEALTH_NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

template <typename T>
__global__ __launch_bounds__(HEALTH_NT) void codebook_health_kernel(const T* __restrict__ n, int64_t K, int64_t stride,
                                                                    float* __restrict__ out3, double* __restrict__ out3_f64,
                                                                    double* __restrict__ total) {
    __shared__ double red[HEALTH_NT];
    const int t = threadIdx.x;
    double s = 0.0, act = 0.0;
    for (int64_t k = t; k < K; k += HEALTH_NT) {           // thread t owns the codes k = t (mod 256), in ascending order
        const double c = (double)n[k * stride];
        s += c;
        act += c > 0.0 ? 1.0 : 0.0;
        if (total != nullptr) total[k] += c;
    }
    const double S = block_sum_f64(s, red);
    const double A = block_sum_f64(act, red);
    double h = 0.0;
    if (S > 0.0)
        for (int64_t k = t; k < K; k += HEALTH_NT) {
            const double c = (double)n[k * stride];
            if (c > 0.0) {
                const double p = c / S;
                h -= p * log(p);
            }
        }
    const double H = block_sum_f64(h, red);
    if (t == 0) {
        const double ppl = S > 0.0 ? exp(H) : 0.0, active = S > 0.0 ? A : 0.0;
        out3[0] = (float)ppl, out3[1] = (float)active, out3[2] = (float)S;
        if (out3_f64 != nullptr) out3_f64[0] = ppl, out3_f64[1] = active, out3_f64[2] = S;
    }
}

}  // namespace

extern "C" {

size_t dvq_scalar_push_state_bytes(int64_t columns) {
    if (columns < 1 || columns > PUSH_COLUMNS_MAX) return 0;
    return (size_t)columns * (sizeof(double) + 2 * sizeof(int64_t) + sizeof(float));
}

int dvq_scalar_push(const dvq_scalar_record* rec, int32_t count, int32_t col0, int32_t columns, void* state, dvq_stream_t stream) {
    DVQ_REQUIRE(rec != nullptr && state != nullptr, DVQ_EINVAL, "dvq_scalar_push: null pointer");
    DVQ_REQUIRE(columns >= 1 && columns <= PUSH_COLUMNS_MAX, DVQ_ESHAPE, "dvq_scalar_push: %d columns, 1 .. %d supported", columns,
                PUSH_COLUMNS_MAX);
    DVQ_REQUIRE(count >= 1 && count <= PUSH_MAX, DVQ_ESHAPE, "dvq_scalar_push: %d scalars in one launch, 1 .. %d supported", count, PUSH_MAX);
    DVQ_REQUIRE(col0 >= 0 && col0 + count <= columns, DVQ_ESHAPE, "dvq_scalar_push: columns %d .. %d outside a state block of %d", col0,
                col0 + count - 1, columns);
    DVQ_REQUIRE(((uintptr_t)state & 7) == 0, DVQ_EINVAL, "dvq_scalar_push: state must be 8-byte aligned");
    for (int i = 0; i < count; ++i) {
        const int code = rec->code[i];
        DVQ_REQUIRE(code >= DVQ_SCALAR_F32 && code <= DVQ_SCALAR_SKIP, DVQ_EINVAL, "dvq_scalar_push: scalar %d has type code %d", i, code);
        if (code == DVQ_SCALAR_IMM || code == DVQ_SCALAR_SKIP) continue;
        const uint64_t align = code == DVQ_SCALAR_BF16 ? 1 : (code == DVQ_SCALAR_F32 || code == DVQ_SCALAR_I32) ? 3 : 7;
        DVQ_REQUIRE(rec->addr[i] != 0 && (rec->addr[i] & align) == 0, DVQ_EINVAL, "dvq_scalar_push: scalar %d: null or misaligned address", i);
    }
    scalar_push_kernel<<<dim3(1), dim3(PUSH_MAX), 0, (hipStream_t)stream>>>(*rec, count, col0, columns, state);
    DVQ_CHECK_LAUNCH("scalar_push");
    return DVQ_OK;
}

int dvq_codebook_health(const void* counts, int counts_type, int64_t K, int64_t stride, float* out3, double* out3_f64, double* total,
                        dvq_stream_t stream) {
    DVQ_REQUIRE(counts != nullptr && out3 != nullptr, DVQ_EINVAL, "dvq_codebook_health: null pointer");
    DVQ_REQUIRE(counts_type == DVQ_SCALAR_F32 || counts_type == DVQ_SCALAR_I64, DVQ_EINVAL,
                "dvq_codebook_health: counts are fp32 (DVQ_SCALAR_F32) or int64 (DVQ_SCALAR_I64)");
    DVQ_REQUIRE(K >= 1 && K <= (1 << 24) && stride >= 1 && stride <= (1 << 24), DVQ_ESHAPE, "dvq_codebook_health: K and stride must be in 1 .. 2^24");
    DVQ_REQUIRE(((uintptr_t)counts & (counts_type == DVQ_SCALAR_F32 ? 3 : 7)) == 0 && ((uintptr_t)out3 & 3) == 0 &&
                    (((uintptr_t)out3_f64 | (uintptr_t)total) & 7) == 0,
                DVQ_EINVAL, "dvq_codebook_health: misaligned pointer");
    if (counts_type == DVQ_SCALAR_F32)
        codebook_health_kernel<float><<<dim3(1), dim3(HEALTH_NT), 0, (hipStream_t)stream>>>((const float*)counts, K, stride, out3, out3_f64, total);
    else
        codebook_health_kernel<int64_t><<<dim3(1), dim3(HEALTH_NT), 0, (hipStream_t)stream>>>((const int64_t*)counts, K, stride, out3, out3_f64, total);
    DVQ_CHECK_LAUNCH("codebook_health");
    return DVQ_OK;
}

}  // extern "C"
