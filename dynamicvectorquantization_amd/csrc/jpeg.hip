// Device stage of the JPEG decode (docs/design/23-device-jpeg.md): everything after the Huffman pass (csrc/jpeg_host.cpp), for a whole
// batch of differently sized images in two launches, pixel for pixel what libjpeg-turbo's default path produces:
//   (a) jpeg_idct_kernel   dequantise, 8x8 inverse DCT (jidctint.c's "islow": 13-bit constants, 32-bit integers), + 128, clamp
//                          -> uint8 component planes, each as large as its block grid padded to whole MCUs
//   (b) jpeg_color_kernel  fancy (triangle-filter) chroma upsampling on the UNPADDED chroma planes with edge replication
//                          (jdsample.c: h2v1_fancy_upsample, h2v2_fancy_upsample), YCbCr -> RGB in 16-bit fixed point (jdcolor.c),
//                          packed uint8 [h][w][3] -- the buffer dvq_image_batch_transform reads
// Both kernels walk a flat list of work items (32 blocks / 1024 pixels, counted per image so that an item never spans two images);
// each descriptor carries the prefix sum of the items before it, a workgroup finds its image by bisection.  The grids are fixed:
// the launcher never reads the descriptors, which live in device memory.
#include "dvq_common.h"

namespace {

struct JpegDesc {
    int64_t coef_off;       // int16 elements into coef (a multiple of 64)
    int64_t plane_off;      // bytes into planes_tmp (a multiple of 16)
    int64_t rgb_off;        // bytes into rgb_out (a multiple of 4)
    int32_t w, h;
    int32_t ncomp;          // 1, 3, or 0: not decoded here (no items)
    int32_t hs, vs;         // luma sampling factors: 1x1, 2x1 or 2x2 (chroma is 1x1)
    int32_t mcux, mcuy;     // MCU grid
    int32_t idct_item0, idct_items;      // kernel (a): items of all images before this one, items of this one = ceil(blocks / 32)
    int32_t pix_item0, pix_items;        // kernel (b): the same in items of 1024 pixels
    int32_t pad[3];
    uint16_t q[3][64];      // quantisation tables per component, natural order (at byte 80: rows are 16-byte aligned)
};
static_assert(sizeof(JpegDesc) == 464 && offsetof(JpegDesc, q) == 80, "JpegDesc layout");

constexpr int IDCT_BLOCKS = 32;        // per item: 256 threads, 8 lanes per block
constexpr int PIX_PER_THREAD = 4;
constexpr int PIX_ITEM = 256 * PIX_PER_THREAD;
constexpr int GRID = 1024;             // workgroups per launch: 4 per CU; larger batches loop

// largest i with item0(i) <= item: images without items share their prefix with the next image and are passed over
template <bool IDCT>
__device__ __forceinline__ int find_image(const JpegDesc* __restrict__ desc, int B, int item) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int first = IDCT ? desc[mid].idct_item0 : desc[mid].pix_item0;
        if (first <= item) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

#define DVQ_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

// one 8-point inverse DCT of jidctint.c (jpeg_idct_islow), results descaled by `SHIFT` bits
template <int SHIFT>
__device__ __forceinline__ void idct8(const int (&c)[8], int (&o)[8]) {
    // even part
    const int z1 = (c[2] + c[6]) * 4433;
    const int t2 = z1 - c[6] * 15137;
    const int t3 = z1 + c[2] * 6270;
    const int t0 = (c[0] + c[4]) * 8192;
    const int t1 = (c[0] - c[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    // odd part
    int a0 = c[7], a1 = c[5], a2 = c[3], a3 = c[1];
    int y1 = a0 + a3, y2 = a1 + a2, y3 = a0 + a2, y4 = a1 + a3;
    const int y5 = (y3 + y4) * 9633;
    a0 *= 2446;
    a1 *= 16819;
    a2 *= 25172;
    a3 *= 12299;
    y1 *= -7373;
    y2 *= -20995;
    y3 = y3 * -16069 + y5;
    y4 = y4 * -3196 + y5;
    a0 += y1 + y3;
    a1 += y2 + y4;
    a2 += y2 + y3;
    a3 += y1 + y4;
    o[0] = DVQ_DESCALE(t10 + a3, SHIFT);
    o[7] = DVQ_DESCALE(t10 - a3, SHIFT);
    o[1] = DVQ_DESCALE(t11 + a2, SHIFT);
    o[6] = DVQ_DESCALE(t11 - a2, SHIFT);
    o[2] = DVQ_DESCALE(t12 + a1, SHIFT);
    o[5] = DVQ_DESCALE(t12 - a1, SHIFT);
    o[3] = DVQ_DESCALE(t13 + a0, SHIFT);
    o[4] = DVQ_DESCALE(t13 - a0, SHIFT);
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// LDS tile of one 8x8 block of ints: rows padded from 8 to 12 dwords (one 16-byte access), blocks from 96 to 104 dwords, so that
// the 16-byte row accesses stay aligned and the 32 lanes of a half wave (4 blocks x 8 columns) reading one row index as single
// dwords have 32 different dword addresses mod 32 (block * 104 + column = block * 8 + column mod 32).  That is address arithmetic
// under the 32-bank rule for single-dword accesses; the conflict counters were not read
constexpr int LDS_ROW = 12, LDS_BLOCK = 8 * LDS_ROW + 8;

// lane (block, j): loads row j of its block's coefficients as one 16-byte vector and dequantises it; the tile is transposed through
// LDS; the lane runs the COLUMN pass on column j (descale 11); transposed back; the lane runs the ROW pass on row j (descale 18),
// adds 128, clamps and stores the 8 pixels of that row as one 8-byte vector
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const JpegDesc* __restrict__ desc, int B,
                                                        uint8_t* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) int tile[IDCT_BLOCKS * LDS_BLOCK];
    const int total = desc[B - 1].idct_item0 + desc[B - 1].idct_items;
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    int* const mine = tile + slot * LDS_BLOCK;
    for (int item = blockIdx.x; item < total; item += gridDim.x) {      // uniform per workgroup: the barriers below are safe
        const int img = find_image<true>(desc, B, item);
        const JpegDesc* d = desc + img;
        const int mcux = d->mcux, mcuy = d->mcuy, hs = d->hs, vs = d->vs, ncomp = d->ncomp;
        const int nY = mcux * hs * mcuy * vs, nC = mcux * mcuy;
        const int nblocks = ncomp == 3 ? nY + 2 * nC : nY;
        const int b = (item - d->idct_item0) * IDCT_BLOCKS + slot;
        const bool active = b < nblocks;
        const int c = b < nY ? 0 : (b < nY + nC ? 1 : 2);
        int x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (active) {
            const uint4 cv = *reinterpret_cast<const uint4*>(coef + d->coef_off + (int64_t)b * 64 + j * 8);
            const uint4 qv = *reinterpret_cast<const uint4*>(&d->q[c][j * 8]);
            const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[2 * k] = (int)(short)(cw[k] & 0xffffu) * (int)(qw[k] & 0xffffu);
                x[2 * k + 1] = (int)(short)(cw[k] >> 16) * (int)(qw[k] >> 16);
            }
        }
        *reinterpret_cast<int4*>(mine + j * LDS_ROW) = make_int4(x[0], x[1], x[2], x[3]);
        *reinterpret_cast<int4*>(mine + j * LDS_ROW + 4) = make_int4(x[4], x[5], x[6], x[7]);
        __syncthreads();
        int col[8], ws[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) col[r] = mine[r * LDS_ROW + j];
        idct8<11>(col, ws);
        // no barrier here: a lane writes back exactly the eight words it has just read (column j of its own block)
#pragma unroll
        for (int r = 0; r < 8; ++r) mine[r * LDS_ROW + j] = ws[r];
        __syncthreads();
        const int4 r0 = *reinterpret_cast<const int4*>(mine + j * LDS_ROW);
        const int4 r1 = *reinterpret_cast<const int4*>(mine + j * LDS_ROW + 4);
        const int row[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
        int px[8];
        idct8<18>(row, px);
        if (active) {
            const int bl = b - (c == 0 ? 0 : (c == 1 ? nY : nY + nC));
            const int bcols = c == 0 ? mcux * hs : mcux;
            const int br = bl / bcols, bc = bl - br * bcols;
            const int64_t plane = d->plane_off + (c == 0 ? 0 : (int64_t)(nY + (c - 1) * nC) * 64);
            uint2 o;
            o.x = (unsigned)clamp8(px[0] + 128) | ((unsigned)clamp8(px[1] + 128) << 8) | ((unsigned)clamp8(px[2] + 128) << 16) |
                  ((unsigned)clamp8(px[3] + 128) << 24);
            o.y = (unsigned)clamp8(px[4] + 128) | ((unsigned)clamp8(px[5] + 128) << 8) | ((unsigned)clamp8(px[6] + 128) << 16) |
                  ((unsigned)clamp8(px[7] + 128) << 24);
            *reinterpret_cast<uint2*>(planes + plane + ((int64_t)(br * 8 + j) * bcols + bc) * 8) = o;
        }
        __syncthreads();      // the tile is rewritten by the next item
    }
}

// one upsampled chroma sample at pixel (x, y) of plane `p` (row pitch `pitch`, real size cw x ch)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(int64_t)y * pitch + x];
    const int cx = x >> 1;
    if (vs == 1) {
        const uint8_t* r = p + (int64_t)y * pitch;
        const int s = r[cx];
        if (cw <= 2) return s;                                  // libjpeg replicates where the plane is too narrow for the filter
        if (x & 1) return cx == cw - 1 ? s : (3 * s + r[cx + 1] + 2) >> 2;
        return cx == 0 ? s : (3 * s + r[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* r0 = p + (int64_t)cy * pitch;
    if (cw <= 2) return r0[cx];
    const int ny = (y & 1) ? (cy + 1 < ch ? cy + 1 : cy) : (cy > 0 ? cy - 1 : cy);      // the nearer neighbour row, replicated at the edges
    const uint8_t* r1 = p + (int64_t)ny * pitch;
    const int cs = 3 * r0[cx] + r1[cx];
    if (x & 1) return cx == cw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

// a thread owns 4 consecutive pixels of the image's flat [h * w] pixel list: 12 bytes, stored as three dwords
__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ planes, const JpegDesc* __restrict__ desc, int B,
                                                         uint8_t* __restrict__ rgb) {
    const int total = desc[B - 1].pix_item0 + desc[B - 1].pix_items;
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int img = find_image<false>(desc, B, item);
        const JpegDesc* d = desc + img;
        const int w = d->w, h = d->h, hs = d->hs, vs = d->vs, mcux = d->mcux, mcuy = d->mcuy, ncomp = d->ncomp;
        const int64_t npix = (int64_t)w * h;
        const int64_t p0 = ((int64_t)(item - d->pix_item0) * 256 + threadIdx.x) * PIX_PER_THREAD;
        if (p0 >= npix) continue;
        const int nY = mcux * hs * mcuy * vs, nC = mcux * mcuy;
        const int pitch_y = mcux * hs * 8, pitch_c = mcux * 8;
        const uint8_t* py = planes + d->plane_off;
        const uint8_t* pcb = py + (int64_t)nY * 64;
        const uint8_t* pcr = pcb + (int64_t)nC * 64;
        const int cw = (w + hs - 1) / hs, ch = (h + vs - 1) / vs;
        uint8_t out[3 * PIX_PER_THREAD];
        int y = (int)(p0 / w), x = (int)(p0 - (int64_t)y * w);
#pragma unroll
        for (int u = 0; u < PIX_PER_THREAD; ++u) {
            int r = 0, g = 0, bl = 0;
            if (p0 + u < npix) {
                const int Y = py[(int64_t)y * pitch_y + x];
                if (ncomp == 3) {
                    const int cb = chroma_at(pcb, pitch_c, cw, ch, hs, vs, x, y) - 128;
                    const int cr = chroma_at(pcr, pitch_c, cw, ch, hs, vs, x, y) - 128;
                    // jdcolor.c: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554
                    r = clamp8(Y + ((91881 * cr + 32768) >> 16));
                    g = clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
                    bl = clamp8(Y + ((116130 * cb + 32768) >> 16));
                } else {
                    r = g = bl = Y;
                }
            }
            out[3 * u] = (uint8_t)r;
            out[3 * u + 1] = (uint8_t)g;
            out[3 * u + 2] = (uint8_t)bl;
            if (++x == w) {
                x = 0;
                ++y;
            }
        }
        uint8_t* o = rgb + d->rgb_off + p0 * 3;
        if (p0 + PIX_PER_THREAD <= npix) {
            unsigned* o32 = reinterpret_cast<unsigned*>(o);      // rgb_off % 4 == 0 and p0 * 3 % 12 == 0
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o32[k] = (unsigned)out[4 * k] | ((unsigned)out[4 * k + 1] << 8) | ((unsigned)out[4 * k + 2] << 16) |
                         ((unsigned)out[4 * k + 3] << 24);
        } else {
            const int nb = (int)(npix - p0) * 3;
            for (int k = 0; k < nb; ++k) o[k] = out[k];
        }
    }
}

}  // namespace

extern "C" {

size_t dvq_jpeg_desc_bytes(void) { return sizeof(JpegDesc); }

int dvq_jpeg_batch_decode(const int16_t* coef, const void* desc, int64_t B, uint8_t* planes_tmp, uint8_t* rgb_out, dvq_stream_t stream) {
    DVQ_REQUIRE(coef && desc && planes_tmp && rgb_out, DVQ_EINVAL, "dvq_jpeg_batch_decode: null pointer");
    DVQ_REQUIRE(B > 0 && B <= 65535, DVQ_ESHAPE, "dvq_jpeg_batch_decode: bad batch size B=%lld", (long long)B);
    DVQ_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)desc & 15) == 0 && ((uintptr_t)planes_tmp & 15) == 0 &&
                    ((uintptr_t)rgb_out & 3) == 0,
                DVQ_EINVAL, "dvq_jpeg_batch_decode: coef, desc and planes_tmp must be 16-byte aligned, rgb_out 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    jpeg_idct_kernel<<<dim3(GRID), dim3(256), 0, s>>>(coef, (const JpegDesc*)desc, (int)B, planes_tmp);
    DVQ_CHECK_LAUNCH("jpeg_idct");
    jpeg_color_kernel<<<dim3(GRID), dim3(256), 0, s>>>(planes_tmp, (const JpegDesc*)desc, (int)B, rgb_out);
    DVQ_CHECK_LAUNCH("jpeg_color");
    return DVQ_OK;
}

}  // extern "C"
