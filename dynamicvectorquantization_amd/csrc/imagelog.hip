// Training-time image logging (gfx950): the panels a log event draws and the 8-bit grid it writes, made from tensors that are already
// on the device.  Counterparts in the reference run on the host: modules/dynamic_modules/utils.py:41-161 (per-image PIL blends, a Python
// triple loop over grain cells) and utils/logger.py:137-147 (torchvision make_grid on fp32 CPU copies).
//
// The arithmetic is the reference's, step for step in fp32 (docs/design/18-image-logging.md): every product, sum and quotient below
// is rounded on its own -- this file is compiled with -ffp-contract=off (build.py) and the pragma below says the same -- and every
// division is an IEEE division, never a reciprocal multiply.  Float -> byte conversions truncate.  The only reductions are minima and
// maxima, so no result depends on an order: a kernel's output is a pure function of its inputs, bit for bit.
//
// Min / max: PARTS workgroups per segment (an image for the overlay, the whole tensor for the grid) write partial extrema into the
// caller's workspace; the compose kernel's workgroups each fold the PARTS partials of their segment again (PARTS loads, one LDS round)
// instead of a third launch.  No float atomics.
#include "dvq_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int PARTS = 256;                      // partial extrema per segment; == NT: the compose kernels fold them one per thread
constexpr int NW = NT / DVQ_WAVE;

__device__ __forceinline__ float clamp11(float v, int clamp) { return clamp ? fminf(fmaxf(v, -1.0f), 1.0f) : v; }

// workgroup-wide (min, max) of each thread's (lo, hi); every thread gets the result
__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
    __shared__ float red[NW][2];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const int wid = threadIdx.x / DVQ_WAVE;
    if ((threadIdx.x % DVQ_WAVE) == 0) {
        red[wid][0] = lo;
        red[wid][1] = hi;
    }
    __syncthreads();
    lo = red[0][0];
    hi = red[0][1];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        lo = fminf(lo, red[w][0]);
        hi = fmaxf(hi, red[w][1]);
    }
}

// grid (PARTS, segments): partial[(seg * PARTS + part) * 2 + {0, 1}] = min / max of that part of the segment (+inf / -inf if empty)
__global__ __launch_bounds__(NT) void minmax_partial_kernel(const float* __restrict__ x, int64_t seg_len, int64_t chunk, int clamp,
                                                            float* __restrict__ partial) {
    const int64_t seg = blockIdx.y, part = blockIdx.x;
    const float* xs = x + seg * seg_len;
    const int64_t e0 = part * chunk;
    const int64_t e1 = e0 + chunk < seg_len ? e0 + chunk : seg_len;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += NT) {
        const float v = clamp11(xs[e], clamp);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        partial[(seg * PARTS + part) * 2 + 0] = lo;
        partial[(seg * PARTS + part) * 2 + 1] = hi;
    }
}

// (lo, d) of a segment from its partials: d = float32(max(double(hi) - double(lo), 1e-5)), the divisor of image_normalize / make_grid
__device__ __forceinline__ void segment_range(const float* __restrict__ partial, int64_t seg, float& lo, float& d) {
    float a = partial[(seg * PARTS + threadIdx.x) * 2 + 0];
    float b = partial[(seg * PARTS + threadIdx.x) * 2 + 1];
    block_minmax(a, b);
    double dd = (double)b - (double)a;
    if (!(dd > 1e-5)) dd = 1e-5;
    lo = a;
    d = (float)dd;
}

__device__ __forceinline__ unsigned char unit_to_byte(float v, float lo, float d) {
    const float g = (v - lo) / d;
    return (unsigned char)(int)(g * 255.0f);
}

struct Rgb {
    int c[3];
};

// grid (ceil(H * W / NT), B): one thread per pixel, its three channels
__global__ __launch_bounds__(NT) void grain_overlay_kernel(const float* __restrict__ x, const int64_t* __restrict__ grain,
                                                           const float* __restrict__ score, int levels, int64_t H, int64_t W, int64_t h,
                                                           int64_t w, int64_t cell, Rgb low, Rgb high, float scaler,
                                                           const float* __restrict__ partial, float* __restrict__ out) {
    const int64_t b = blockIdx.y;
    float lo, d;
    segment_range(partial, b, lo, d);
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= H * W) return;
    const int64_t y = p / W, xx = p % W;
    const int64_t ci = b * h * w + (y / cell) * w + xx / cell;
    int col[3];
    if (grain != nullptr && levels == 2) {      // integer arithmetic of the reference: high * s + low * (1 - s), wrapped to a byte
        const int64_t s = grain[ci];
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c] = (int)((unsigned long long)((int64_t)high.c[c] * s + (int64_t)low.c[c] * (1 - s)) & 0xffu);
    } else {
        const float s = grain != nullptr ? (float)grain[ci] / 2.0f : score[ci];
        const float t = 1.0f - s;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float hs = (float)high.c[c] * s;
            const float lt = (float)low.c[c] * t;
            col[c] = (int)(unsigned char)(int)(hs + lt);
        }
    }
    const float* xb = x + b * 3 * H * W;
    float* ob = out + b * 3 * H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = (int)unit_to_byte(xb[c * H * W + p], lo, d);
        const float step = scaler * (float)(col[c] - a);        // Image.blend: a + alpha * (b - a) in fp32, truncated
        const int k = (int)(unsigned char)(int)((float)a + step);
        ob[c * H * W + p] = (float)k / 255.0f;
    }
}

__device__ __forceinline__ bool on_line(int64_t l, int64_t cell, int64_t g) {
    if (l == 0) return true;
    if (g >= 1 && l == cell / 2) return true;
    if (g == 2 && (l == cell / 4 || l == cell - cell / 4)) return true;
    return false;
}

// grid (ceil(H * W / NT), B): a pixel on a line of its cell gets -1 in all three channels, every other pixel is left alone
__global__ __launch_bounds__(NT) void grain_lines_kernel(float* __restrict__ x, const int64_t* __restrict__ grain, int64_t H, int64_t W,
                                                         int64_t h, int64_t w, int64_t cell) {
    const int64_t b = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= H * W) return;
    const int64_t y = p / W, xx = p % W;
    const int64_t g = grain[b * h * w + (y / cell) * w + xx / cell];
    if (!(on_line(y % cell, cell, g) || on_line(xx % cell, cell, g))) return;
    float* xb = x + b * 3 * H * W + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) xb[c * H * W] = -1.0f;
}

// one thread per grid pixel, its three bytes (a one-channel input is repeated, as make_grid does)
__global__ __launch_bounds__(NT) void image_grid_u8_kernel(const float* __restrict__ x, int64_t N, int64_t C, int64_t H, int64_t W,
                                                           int64_t xmaps, int64_t padding, int64_t GH, int64_t GW, int clamp,
                                                           const float* __restrict__ partial, unsigned char* __restrict__ out) {
    float lo, d;
    segment_range(partial, 0, lo, d);
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= GH * GW) return;
    const int64_t gy = p / GW, gx = p % GW;
    int64_t k = 0, iy = gy, ix = gx;
    bool inside = true;
    if (N > 1) {
        const int64_t ch = H + padding, cw = W + padding;
        const int64_t r = gy / ch, q = gx / cw;
        iy = gy % ch - padding;
        ix = gx % cw - padding;
        k = r * xmaps + q;
        inside = iy >= 0 && ix >= 0 && q < xmaps && k < N;       // r past the last row gives k >= N
    }
    unsigned char* o = out + p * 3;
    if (!inside) {
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const float* xi = x + (k * C * H + iy) * W + ix;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = unit_to_byte(clamp11(xi[(C == 3 ? c : 0) * H * W], clamp), lo, d);
}

int launch_minmax(const float* x, int64_t segments, int64_t seg_len, int clamp, float* partial, hipStream_t s) {
    const int64_t chunk = cdiv64(seg_len, PARTS);
    minmax_partial_kernel<<<dim3(PARTS, (unsigned)segments), dim3(NT), 0, s>>>(x, seg_len, chunk, clamp, partial);
    DVQ_CHECK_LAUNCH("minmax_partial");
    return DVQ_OK;
}

Rgb unpack_rgb(uint32_t v) {
    Rgb r;
    r.c[0] = (int)((v >> 16) & 0xffu);
    r.c[1] = (int)((v >> 8) & 0xffu);
    r.c[2] = (int)(v & 0xffu);
    return r;
}

// cell size of a grain map [h, w] over an image [H, W]; 0 if the map does not tile the image in squares
int64_t grain_cell(int64_t H, int64_t W, int64_t h, int64_t w) {
    if (h <= 0 || w <= 0 || H <= 0 || W <= 0 || H % h != 0 || W % w != 0 || H / h != W / w) return 0;
    return H / h;
}

constexpr int64_t MAX_ELEMS = 1ll << 31;        // a log event moves a handful of images: larger tensors are refused, not indexed
constexpr int64_t MAX_BATCH = 65535;            // gridDim.y

}  // namespace

extern "C" size_t dvq_imagelog_workspace_bytes(int64_t segments) {
    if (segments <= 0) return 0;
    return (size_t)segments * PARTS * 2 * sizeof(float);
}

extern "C" int dvq_grain_overlay(const float* x, const int64_t* grain, const float* score, int levels, int64_t B, int64_t H, int64_t W,
                                 int64_t h, int64_t w, uint32_t low_rgb, uint32_t high_rgb, float scaler, float* out, void* ws,
                                 size_t ws_bytes, dvq_stream_t stream) {
    DVQ_REQUIRE(x && out && ws, DVQ_EINVAL, "dvq_grain_overlay: null pointer");
    DVQ_REQUIRE((grain != nullptr) != (score != nullptr), DVQ_EINVAL, "dvq_grain_overlay: pass a grain map or a score map, not both or neither");
    DVQ_REQUIRE(score != nullptr || levels == 2 || levels == 3, DVQ_EINVAL, "dvq_grain_overlay: levels=%d is not 2 or 3", levels);
    DVQ_REQUIRE(scaler >= 0.0f && scaler <= 1.0f, DVQ_EINVAL, "dvq_grain_overlay: scaler=%g outside [0, 1]", (double)scaler);
    DVQ_REQUIRE(low_rgb <= 0xffffffu && high_rgb <= 0xffffffu, DVQ_EINVAL, "dvq_grain_overlay: colours are 0xRRGGBB");
    const int64_t cell = grain_cell(H, W, h, w);
    DVQ_REQUIRE(B > 0 && B <= MAX_BATCH && cell > 0, DVQ_ESHAPE,
                "dvq_grain_overlay: B=%lld, map %lld x %lld over image %lld x %lld (the map must tile the image in square cells)",
                (long long)B, (long long)h, (long long)w, (long long)H, (long long)W);
    DVQ_REQUIRE(H * W < MAX_ELEMS / (3 * B), DVQ_ESHAPE, "dvq_grain_overlay: %lld x 3 x %lld x %lld elements is too many", (long long)B,
                (long long)H, (long long)W);
    DVQ_REQUIRE(ws_bytes >= dvq_imagelog_workspace_bytes(B), DVQ_EWORKSPACE, "dvq_grain_overlay: workspace %zu bytes < %zu", ws_bytes,
                dvq_imagelog_workspace_bytes(B));
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(ws);
    const int rc = launch_minmax(x, B, 3 * H * W, 0, partial, s);
    if (rc != DVQ_OK) return rc;
    grain_overlay_kernel<<<dim3((unsigned)cdiv64(H * W, NT), (unsigned)B), dim3(NT), 0, s>>>(
        x, grain, score, levels, H, W, h, w, cell, unpack_rgb(low_rgb), unpack_rgb(high_rgb), scaler, partial, out);
    DVQ_CHECK_LAUNCH("grain_overlay");
    return DVQ_OK;
}

extern "C" int dvq_grain_lines(float* x, const int64_t* grain, int levels, int64_t B, int64_t H, int64_t W, int64_t h, int64_t w,
                               dvq_stream_t stream) {
    DVQ_REQUIRE(x && grain, DVQ_EINVAL, "dvq_grain_lines: null pointer");
    DVQ_REQUIRE(levels == 2 || levels == 3, DVQ_EINVAL, "dvq_grain_lines: levels=%d is not 2 or 3", levels);
    const int64_t cell = grain_cell(H, W, h, w);
    DVQ_REQUIRE(B > 0 && B <= MAX_BATCH && cell > 0, DVQ_ESHAPE,
                "dvq_grain_lines: B=%lld, map %lld x %lld over image %lld x %lld (the map must tile the image in square cells)",
                (long long)B, (long long)h, (long long)w, (long long)H, (long long)W);
    DVQ_REQUIRE(H * W < MAX_ELEMS / (3 * B), DVQ_ESHAPE, "dvq_grain_lines: %lld x 3 x %lld x %lld elements is too many", (long long)B,
                (long long)H, (long long)W);
    grain_lines_kernel<<<dim3((unsigned)cdiv64(H * W, NT), (unsigned)B), dim3(NT), 0, (hipStream_t)stream>>>(x, grain, H, W, h, w, cell);
    DVQ_CHECK_LAUNCH("grain_lines");
    return DVQ_OK;
}

extern "C" int dvq_image_grid_shape(int64_t N, int64_t H, int64_t W, int64_t nrow, int64_t padding, int64_t* grid_h, int64_t* grid_w) {
    DVQ_REQUIRE(grid_h && grid_w, DVQ_EINVAL, "dvq_image_grid_shape: null pointer");
    DVQ_REQUIRE(N > 0 && H > 0 && W > 0 && nrow > 0 && padding >= 0, DVQ_ESHAPE,
                "dvq_image_grid_shape: N=%lld H=%lld W=%lld nrow=%lld padding=%lld", (long long)N, (long long)H, (long long)W,
                (long long)nrow, (long long)padding);
    if (N == 1) {                               // make_grid returns a single image as it is
        *grid_h = H;
        *grid_w = W;
        return DVQ_OK;
    }
    const int64_t xmaps = nrow < N ? nrow : N;
    const int64_t ymaps = cdiv64(N, xmaps);
    *grid_h = (H + padding) * ymaps + padding;
    *grid_w = (W + padding) * xmaps + padding;
    return DVQ_OK;
}

extern "C" int dvq_image_grid_u8(const float* x, int64_t N, int64_t C, int64_t H, int64_t W, int64_t nrow, int64_t padding, int clamp,
                                 uint8_t* out, size_t out_bytes, void* ws, size_t ws_bytes, dvq_stream_t stream) {
    DVQ_REQUIRE(x && out && ws, DVQ_EINVAL, "dvq_image_grid_u8: null pointer");
    DVQ_REQUIRE(clamp == 0 || clamp == 1, DVQ_EINVAL, "dvq_image_grid_u8: clamp=%d is not 0 or 1", clamp);
    DVQ_REQUIRE(C == 1 || C == 3, DVQ_ESHAPE, "dvq_image_grid_u8: C=%lld is not 1 or 3", (long long)C);
    DVQ_REQUIRE(N > 0 && H > 0 && W > 0 && N < MAX_ELEMS && H < MAX_ELEMS && W < MAX_ELEMS && nrow > 0 && nrow < MAX_ELEMS && padding >= 0 &&
                    padding < MAX_ELEMS,
                DVQ_ESHAPE, "dvq_image_grid_u8: N=%lld H=%lld W=%lld nrow=%lld padding=%lld", (long long)N, (long long)H, (long long)W,
                (long long)nrow, (long long)padding);
    DVQ_REQUIRE(H * W < MAX_ELEMS / (C * N), DVQ_ESHAPE, "dvq_image_grid_u8: %lld x %lld x %lld x %lld elements is too many", (long long)N,
                (long long)C, (long long)H, (long long)W);
    int64_t GH, GW;
    const int rs = dvq_image_grid_shape(N, H, W, nrow, padding, &GH, &GW);
    if (rs != DVQ_OK) return rs;
    DVQ_REQUIRE(GH < MAX_ELEMS && GW < MAX_ELEMS && GH * GW < MAX_ELEMS / 3, DVQ_ESHAPE, "dvq_image_grid_u8: a %lld x %lld grid is too large",
                (long long)GH, (long long)GW);
    DVQ_REQUIRE(out_bytes >= (size_t)(GH * GW * 3), DVQ_EWORKSPACE, "dvq_image_grid_u8: output %zu bytes < %lld x %lld x 3", out_bytes,
                (long long)GH, (long long)GW);
    DVQ_REQUIRE(ws_bytes >= dvq_imagelog_workspace_bytes(1), DVQ_EWORKSPACE, "dvq_image_grid_u8: workspace %zu bytes < %zu", ws_bytes,
                dvq_imagelog_workspace_bytes(1));
    hipStream_t s = (hipStream_t)stream;
    float* partial = static_cast<float*>(ws);
    const int rc = launch_minmax(x, 1, N * C * H * W, clamp, partial, s);
    if (rc != DVQ_OK) return rc;
    const int64_t xmaps = nrow < N ? nrow : N;
    image_grid_u8_kernel<<<dim3((unsigned)cdiv64(GH * GW, NT)), dim3(NT), 0, s>>>(x, N, C, H, W, xmaps, padding, GH, GW, clamp, partial, out);
    DVQ_CHECK_LAUNCH("image_grid_u8");
    return DVQ_OK;
}
