// Device stage of the PNG decode (docs/design/29-device-png.md): the host inflates the IDAT stream and checks its length and filter
// bytes (data.decode_png_host); the scanlines arrive FILTERED and this file reverses the five PNG filters for a whole batch of
// differently sized images in one launch, pixel for pixel what PIL decodes, and writes packed uint8 [h][w][3] -- the buffer
// dvq_image_batch_transform reads.  Grey goes to all three channels, alpha bytes are dropped: every byte lane of a pixel is a chain
// of its own, so the alpha lane is never reconstructed at all.
//
// Reconstruction is serial along a row (a = the byte of the pixel to the left) and down a column (b = above, c = above left).  A
// workgroup owns an image and walks it in bands of 64 rows.  Wave k (k < 3) reconstructs byte lane k -- R, G, B, or the grey lane alone
// -- with one row of the band per lane, skewed: at step s lane r reconstructs pixel s - r of its row.  b is then what lane r - 1 produced
// one step earlier (one whole-wave DPP shift), c is the b of the step before, a is the lane's own last result.  Lane 0 takes b from
// the finished last row of the band above (read back from the RGB output; zeros for the first band).
//
// Rows have a pitch of 1 + w * bpp bytes (odd for RGB), so nothing is dword aligned on either side.  All four waves move the bytes: per
// chunk of 64 steps they gather the 64 x 64 skewed pixels the chains will visit into an LDS tile of one dword per pixel (the loads of a
// wave run along a row: coalesced; they are issued before the chunk's chain and land behind it), and scatter the tile the chains
// have finished to the output.  Three tiles rotate -- one being filled, one with the chains in it, one being stored -- with one
// __syncthreads() per chunk; there is no other ordering, no flag and no spin.  Tile rows are 65 dwords apart, so a chain's
// accesses (one row per lane, same column) fall on 32 banks per half wave.
#include "dvq_common.h"

namespace {

struct PngDesc {
    int64_t scan_off;       // bytes into scan: h rows of (1 filter byte + w * bpp bytes)
    int64_t rgb_off;        // bytes into rgb_out
    int32_t w, h;
    int32_t bpp;            // 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA
    int32_t pad;
};
static_assert(sizeof(PngDesc) == 32, "PngDesc layout");

constexpr int BAND = 64;                // rows per band: one per lane of a chain wave
constexpr int CHUNK = 64;               // steps per tile
constexpr int TILE_PITCH = CHUNK + 1;   // dwords between tile rows
constexpr int THREADS = 256;
constexpr int MOVES = BAND * CHUNK / THREADS;       // tile pixels per thread
constexpr int STEPS = 8;                // chain steps whose LDS reads are issued together
constexpr int GRID = 1024;              // workgroups per launch; larger batches loop

// lane r takes the value of lane r - 1 (lane 0 gets 0): the DPP whole-wave shift, one vector move
__device__ __forceinline__ int lane_above(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// Thread m handles pixels m, m + 256, ... of the 64 x 64 tile: pixel i is step j = i & 63 of row r = i >> 6, which is pixel
// x = chunk * 64 + j - r of that row (the skew).  Consecutive threads run along a row: their loads and stores are neighbours.
//
// filtered bytes -> registers, one dword per pixel.  Every load of the thread is issued before the first is used: a position outside
// the image loads the first pixel of the band's first row instead (always inside the buffer) and its tile entry is never read
template <int BPP>
__device__ __forceinline__ void gather_load(unsigned (&v)[MOVES], const uint8_t* __restrict__ rows, int64_t pitch, int m, int chunk,
                                            int rows_in, int w) {
#pragma unroll
    for (int it = 0; it < MOVES; ++it) {
        const int i = m + it * THREADS, r = i >> 6, x = chunk * CHUNK + (i & 63) - r;
        const bool ok = r < rows_in && x >= 0 && x < w;
        const uint8_t* s = ok ? rows + r * pitch + (int64_t)x * BPP : rows;
        unsigned q = s[0];
        if (BPP > 1) q |= (unsigned)s[1] << 8;
        if (BPP > 2) q |= (unsigned)s[2] << 16;
        if (BPP > 3) q |= (unsigned)s[3] << 24;
        v[it] = q;
    }
}

// tile -> packed RGB bytes; grey goes to all three channels, the fourth byte lane (alpha) is dropped
__device__ __forceinline__ void scatter_tile(const unsigned* __restrict__ t, uint8_t* __restrict__ dst, int m, int chunk, int row_first,
                                             int rows_in, int w, bool grey) {
    unsigned v[MOVES];
#pragma unroll
    for (int it = 0; it < MOVES; ++it) {
        const int i = m + it * THREADS;
        v[it] = t[(i >> 6) * TILE_PITCH + (i & 63)];
    }
#pragma unroll
    for (int it = 0; it < MOVES; ++it) {
        const int i = m + it * THREADS, r = i >> 6, x = chunk * CHUNK + (i & 63) - r;
        if (r < rows_in && x >= 0 && x < w) {
            uint8_t* o = dst + ((int64_t)(row_first + r) * w + x) * 3;
            o[0] = (uint8_t)v[it];
            o[1] = (uint8_t)(grey ? v[it] : v[it] >> 8);
            o[2] = (uint8_t)(grey ? v[it] : v[it] >> 16);
        }
    }
}

__global__ __launch_bounds__(THREADS) void png_unfilter_kernel(const uint8_t* __restrict__ scan, const PngDesc* __restrict__ desc, int B,
                                                               uint8_t* rgb) {
    __shared__ unsigned tile[3][BAND * TILE_PITCH];
    __shared__ unsigned above[3][CHUNK];        // lane 0's b: the last row of the band above, pixels chunk * 64 ..
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int img = blockIdx.x; img < B; img += gridDim.x) {      // everything below is uniform per workgroup up to the barriers
        const PngDesc d = desc[img];
        const int w = d.w, h = d.h, bpp = d.bpp;
        const int64_t pitch = 1 + (int64_t)w * bpp;
        const uint8_t* src = scan + d.scan_off;
        uint8_t* dst = rgb + d.rgb_off;
        const bool chain = wave < (bpp < 3 ? 1 : 3);            // this wave reconstructs byte lane `wave`; alpha lanes are nobody's
        const int nbands = (h + BAND - 1) / BAND;
        for (int band = 0; band < nbands; ++band) {
            const int row_first = band * BAND;
            const int rows_in = h - row_first < BAND ? h - row_first : BAND;
            const int nchunks = (w + rows_in - 1 + CHUNK - 1) / CHUNK;
            const uint8_t* rows = src + (int64_t)row_first * pitch + 1;
            // chain state of lane r (row row_first + r)
            const bool row_ok = lane < rows_in;
            const int ft = row_ok ? src[(int64_t)(row_first + lane) * pitch] : 0;
            const int m_sub = -(ft == 1), m_up = -(ft == 2), m_avg = -(ft == 3), m_paeth = -(ft == 4), m_row = row_ok ? 255 : 0;
            int a = 0, bprev = 0, res = 0;
            for (int p = 0; p < nchunks + 2; ++p) {
                unsigned g[MOVES];
                if (p < nchunks) {              // the tile the chains enter next phase: loads now, LDS writes after the chain
                    if (bpp == 1) gather_load<1>(g, rows, pitch, tid, p, rows_in, w);
                    else if (bpp == 2) gather_load<2>(g, rows, pitch, tid, p, rows_in, w);
                    else if (bpp == 3) gather_load<3>(g, rows, pitch, tid, p, rows_in, w);
                    else gather_load<4>(g, rows, pitch, tid, p, rows_in, w);
                }
                const int k = p - 1;
                if (chain && k >= 0 && k < nchunks) {
                    uint8_t* tb = reinterpret_cast<uint8_t*>(tile[k % 3] + lane * TILE_PITCH) + wave;
                    const uint8_t* ab = reinterpret_cast<const uint8_t*>(above[k % 3]) + wave;
                    for (int j0 = 0; j0 < CHUNK; j0 += STEPS) {
                        int f[STEPS], up[STEPS];        // the LDS reads of STEPS steps, issued ahead of the dependent chain
#pragma unroll
                        for (int u = 0; u < STEPS; ++u) {
                            f[u] = tb[(j0 + u) * 4];
                            up[u] = ab[(j0 + u) * 4];
                        }
#pragma unroll
                        for (int u = 0; u < STEPS; ++u) {
                            const int x = k * CHUNK + j0 + u - lane;
                            int b = lane_above(res);
                            if (lane == 0) b = band > 0 ? up[u] : 0;
                            const int c = bprev;
                            bprev = b;
                            // straight-line on purpose: every predictor is computed and picked by the row's masks, and a lane
                            // outside its row (x < 0, x >= w, a row past the image) produces 0 into a tile entry nobody reads
                            const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
                            const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                            const int pred = (a & m_sub) | (b & m_up) | (((a + b) >> 1) & m_avg) | (paeth & m_paeth);
                            res = (f[u] + pred) & ((unsigned)x < (unsigned)w ? m_row : 0);
                            tb[(j0 + u) * 4] = (uint8_t)res;
                            a = res;
                        }
                    }
                }
                const int ks = p - 2;           // scatter the tile the chains finished one phase ago
                if (ks >= 0 && ks < nchunks) scatter_tile(tile[ks % 3], dst, tid, ks, row_first, rows_in, w, bpp < 3);
                if (p < nchunks) {
                    unsigned* t = tile[p % 3];
#pragma unroll
                    for (int it = 0; it < MOVES; ++it) {
                        const int i = tid + it * THREADS;
                        t[(i >> 6) * TILE_PITCH + (i & 63)] = g[it];
                    }
                    if (band > 0 && tid < CHUNK) {
                        const int x = p * CHUNK + tid;
                        unsigned v = 0;
                        if (x < w) {
                            const uint8_t* s = dst + ((int64_t)(row_first - 1) * w + x) * 3;
                            v = bpp < 3 ? (unsigned)s[0] : ((unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16));
                        }
                        above[p % 3][tid] = v;
                    }
                }
                __syncthreads();
            }
            // the next band reads this band's last row back from the output
            __threadfence();
            __syncthreads();
            __threadfence();
        }
    }
}

}  // namespace

extern "C" {

size_t dvq_png_desc_bytes(void) { return sizeof(PngDesc); }

int dvq_png_batch_unfilter(const uint8_t* scan, const void* desc, int64_t B, uint8_t* rgb_out, dvq_stream_t stream) {
    DVQ_REQUIRE(scan && desc && rgb_out, DVQ_EINVAL, "dvq_png_batch_unfilter: null pointer");
    DVQ_REQUIRE(B > 0 && B <= 65535, DVQ_ESHAPE, "dvq_png_batch_unfilter: bad batch size B=%lld", (long long)B);
    DVQ_REQUIRE(((uintptr_t)desc & 7) == 0, DVQ_EINVAL, "dvq_png_batch_unfilter: desc must be 8-byte aligned");
    png_unfilter_kernel<<<dim3((unsigned)(B < GRID ? B : GRID)), dim3(THREADS), 0, (hipStream_t)stream>>>(scan, (const PngDesc*)desc, (int)B,
                                                                                                    rgb_out);
    DVQ_CHECK_LAUNCH("png_unfilter");
    return DVQ_OK;
}

}  // extern "C"
