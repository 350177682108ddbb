// Reconstruction metrics of a DQ-VAE evaluation (gfx950): per-image MSE / L1 / SSIM of a target and a reconstruction, and the
// grain-aware code histogram (how often each codebook entry is spent as a token).  No counterpart kernel in the reference: its
// codebook-usage tool collects the code map on the host (scripts/tools/codebook_usage_dqvae.py:52-69); SSIM follows Wang et al.
// 2004 (11 x 11 Gaussian window, sigma 1.5, K1 = 0.01, K2 = 0.03, "valid" positions only).
//
// dvq_recon_metrics: one workgroup per (image, channel, tile).  A tile OWNS the input pixels [r0, r0+16) x [c0, c0+64) -- their
// squared / absolute errors -- and the SSIM positions with the same top-left corners; it stages its rows and columns plus the
// 10-pixel halo of both images in LDS (float4 reads when W % 4 == 0), runs the horizontal then the vertical 11-tap pass of the five
// moment maps, and writes its three sums (fp64) into a slab.  A fold kernel adds the slab of each image in a fixed order: no float
// atomics, so the per-image values are bitwise reproducible and do not depend on the other images of the batch.
// dvq_code_histogram: one workgroup per image, integer atomics only (exact, order-independent).
// dvq_recon_cells: the same staging and moment arithmetic with tiles that follow an hg x wg cell grid; the per-pixel values are folded
// per cell piece by one owner each, then per cell over channels and parts (docs/design/30-cell-maps.md).
#include "dvq_common.h"

#include <math.h>

namespace {

constexpr int TH = 16, TW = 64;                 // output tile (rows x columns); TW is one wave wide
constexpr int HALO = 10;                        // 11-tap window
constexpr int RH = TH + HALO, RW = TW + HALO;   // staged region: 26 x 74
constexpr int RWP = 76;                         // LDS row stride of the staged images (16-B aligned rows for the float4 stores)
constexpr int NT = 256;

struct Gauss11 {
    float g[11];
};

// v01 = clamp(v * 0.5 + 0.5, 0, 1) [, floor(v01 * 255 + 0.5) / 255] in fp64: every step is exact for fp32 inputs except the final
// division, which is correctly rounded -- the same value an fp64 restatement on the host computes
__device__ __forceinline__ double to01(float v, int quantize_u8) {
    double d = (double)v * 0.5 + 0.5;
    d = fmin(fmax(d, 0.0), 1.0);
    if (quantize_u8) d = floor(d * 255.0 + 0.5) / 255.0;
    return d;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void recon_metrics_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t H,
                                                                 int64_t W, int tiles_x, int ntiles, int quantize_u8, Gauss11 gw,
                                                                 double* __restrict__ slab) {
    // staged images hold v01 - 0.5: the moments of the shifted values carry a quarter of the cancellation error of
    // E[v^2] - mu^2 that the raw [0, 1] values would
    __shared__ __attribute__((aligned(16))) float sx[RH][RWP];
    __shared__ __attribute__((aligned(16))) float sy[RH][RWP];
    __shared__ float hp[5][RH][TW];             // horizontal pass: mu_x, mu_y, E[x^2], E[y^2], E[xy] per staged row
    __shared__ double red[NT / DVQ_WAVE][3];
    const int64_t blk = blockIdx.x;
    const int tile = (int)(blk % ntiles);
    const int64_t plane = blk / ntiles;         // b * 3 + c
    const int64_t r0 = (int64_t)(tile / tiles_x) * TH, c0 = (int64_t)(tile % tiles_x) * TW;
    const float* xp = x + plane * H * W;
    const float* yp = y + plane * H * W;
    const int tid = threadIdx.x;
    double sq = 0.0, ab = 0.0, ss = 0.0;

    auto stage = [&](int lr, int lc, float xv, float yv) {
        const double ax = to01(xv, quantize_u8), ay = to01(yv, quantize_u8);
        sx[lr][lc] = (float)(ax - 0.5);
        sy[lr][lc] = (float)(ay - 0.5);
        if (lr < TH && lc < TW) {               // owned pixel
            const double d = ax - ay;
            sq += d * d;
            ab += fabs((double)xv - (double)yv);
        }
    };
    if (VEC) {
        constexpr int QW = RWP / 4;             // 19 float4 per staged row (the last covers columns 72..75)
        for (int t = tid; t < RH * QW; t += NT) {
            const int lr = t / QW, lc = (t % QW) * 4;
            const int64_t gr = r0 + lr, gc = c0 + lc;
            if (gr < H && gc < W) {             // W % 4 == 0: the whole float4 lies inside the row
                const float4 a = *reinterpret_cast<const float4*>(xp + gr * W + gc);
                const float4 b = *reinterpret_cast<const float4*>(yp + gr * W + gc);
                stage(lr, lc + 0, a.x, b.x);
                stage(lr, lc + 1, a.y, b.y);
                stage(lr, lc + 2, a.z, b.z);
                stage(lr, lc + 3, a.w, b.w);
            } else {
                *reinterpret_cast<float4*>(&sx[lr][lc]) = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(&sy[lr][lc]) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    } else {
        for (int t = tid; t < RH * RW; t += NT) {
            const int lr = t / RW, lc = t % RW;
            const int64_t gr = r0 + lr, gc = c0 + lc;
            if (gr < H && gc < W) {
                stage(lr, lc, xp[gr * W + gc], yp[gr * W + gc]);
            } else {
                sx[lr][lc] = 0.f;
                sy[lr][lc] = 0.f;
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < RH * TW; t += NT) {   // horizontal pass over every staged row
        const int r = t / TW, j = t % TW;
        float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float a = sx[r][j + k], b = sy[r][j + k], g = gw.g[k];
            mx += g * a;
            my += g * b;
            mxx += g * (a * a);
            myy += g * (b * b);
            mxy += g * (a * b);
        }
        hp[0][r][j] = mx;
        hp[1][r][j] = my;
        hp[2][r][j] = mxx;
        hp[3][r][j] = myy;
        hp[4][r][j] = mxy;
    }
    __syncthreads();
    const int64_t Ho = H - HALO, Wo = W - HALO;
    constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    for (int t = tid; t < TH * TW; t += NT) {   // vertical pass + the SSIM map of the tile's valid positions
        const int i = t / TW, j = t % TW;
        if (r0 + i >= Ho || c0 + j >= Wo) continue;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float g = gw.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += g * hp[q][i + k][j];
        }
        const float vx = m[2] - m[0] * m[0], vy = m[3] - m[1] * m[1], cxy = m[4] - m[0] * m[1];
        const float ux = m[0] + 0.5f, uy = m[1] + 0.5f;
        const float num = (2.f * ux * uy + C1) * (2.f * cxy + C2);
        const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
        ss += (double)(num / den);
    }
    sq = wave_sum(sq);
    ab = wave_sum(ab);
    ss = wave_sum(ss);
    const int wid = tid / DVQ_WAVE;
    if ((tid % DVQ_WAVE) == 0) {
        red[wid][0] = sq;
        red[wid][1] = ab;
        red[wid][2] = ss;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NT / DVQ_WAVE; ++w) s += red[w][tid];
        slab[blk * 3 + tid] = s;
    }
}

// one wave per image: its 3 * ntiles slab entries in a fixed order
__global__ __launch_bounds__(DVQ_WAVE) void recon_metrics_fold_kernel(const double* __restrict__ slab, int64_t per_image,
                                                                      double inv_pix, double inv_pos, double* __restrict__ mse,
                                                                      double* __restrict__ l1, double* __restrict__ ssim) {
    const int64_t b = blockIdx.x;
    const double* s = slab + b * per_image * 3;
    double sq = 0.0, ab = 0.0, ss = 0.0;
    for (int64_t e = threadIdx.x; e < per_image; e += DVQ_WAVE) {
        sq += s[e * 3 + 0];
        ab += s[e * 3 + 1];
        ss += s[e * 3 + 2];
    }
    sq = wave_sum(sq);
    ab = wave_sum(ab);
    ss = wave_sum(ss);
    if (threadIdx.x == 0) {
        mse[b] = sq * inv_pix;
        l1[b] = ab * inv_pix;
        ssim[b] = ss * inv_pos;
    }
}

// ---- per-cell maps (docs/design/30-cell-maps.md) ---------------------------------------------------------------------------------
// The image is cut into hg x wg cells of ch x cw pixels.  Per axis the tiles follow the cells: a cell no longer than the tile edge T
// shares a tile with T / c - 1 neighbours (cpt cells per tile), a longer one is cut into `sub` parts of at most T pixels.  A tile
// therefore holds whole cells or one part of one cell per axis, and a cell's value is the sum of sub_r * sub_c * 3 slab entries.
struct CellAxis {
    int cell;       // pixels per cell
    int cpt;        // cells per tile
    int sub;        // parts per cell
    int ntile;      // tiles on the axis
};

struct CellGeom {
    CellAxis r, c;
    int hg, wg;
};

template <bool VEC>
__global__ __launch_bounds__(NT) void recon_cells_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t H,
                                                               int64_t W, CellGeom gm, int quantize_u8, Gauss11 gw,
                                                               double* __restrict__ slab) {
    // the same staging and fp32 moment arithmetic as recon_metrics_tile_kernel; the per-pixel values stay in LDS and are folded per
    // cell piece in a fixed order (row segments, then the rows of a piece) instead of per tile
    __shared__ __attribute__((aligned(16))) float simg[2][RH][RWP];     // x and y (v01 - 0.5); later the SSIM map of the tile
    __shared__ __attribute__((aligned(16))) float hp[5][RH][TW];        // first the fp64 error maps + row partials, then the moments
    static_assert(sizeof(float) * 5 * RH * TW >= sizeof(double) * 4 * TH * TW, "error maps and row partials share hp");
    static_assert(sizeof(float) * 2 * RH * RWP >= sizeof(float) * TH * TW, "the SSIM map shares the staged images");
    float(*sx)[RWP] = simg[0];
    float(*sy)[RWP] = simg[1];
    double(*dsq)[TW] = reinterpret_cast<double(*)[TW]>(&hp[0][0][0]);
    double(*dab)[TW] = dsq + TH;
    double(*rp0)[TW] = dab + TH;                // row partials [TH][pieces per row]
    double(*rp1)[TW] = rp0 + TH;
    float(*ssm)[TW] = reinterpret_cast<float(*)[TW]>(&simg[0][0][0]);
    const int64_t blk = blockIdx.x;
    const int ntiles = gm.r.ntile * gm.c.ntile;
    const int tile = (int)(blk % ntiles);
    const int64_t plane = blk / ntiles;         // b * 3 + c
    const int tr = tile / gm.c.ntile, tc = tile % gm.c.ntile;
    // origin and owned extent of the tile on each axis
    const int r0 = gm.r.sub == 1 ? tr * gm.r.cpt * gm.r.cell : (tr / gm.r.sub) * gm.r.cell + (tr % gm.r.sub) * TH;
    const int c0 = gm.c.sub == 1 ? tc * gm.c.cpt * gm.c.cell : (tc / gm.c.sub) * gm.c.cell + (tc % gm.c.sub) * TW;
    const int er = gm.r.sub == 1 ? min(gm.r.cpt * gm.r.cell, (int)H - r0) : min(TH, gm.r.cell - (tr % gm.r.sub) * TH);
    const int ec = gm.c.sub == 1 ? min(gm.c.cpt * gm.c.cell, (int)W - c0) : min(TW, gm.c.cell - (tc % gm.c.sub) * TW);
    const int ph = min(gm.r.cell, TH), pw = min(gm.c.cell, TW);          // piece = a cell's share of the tile
    const int npr = (er + ph - 1) / ph, npc = (ec + pw - 1) / pw;
    const int ppt = gm.r.cpt * gm.c.cpt;
    double* out = slab + blk * ppt * 3;
    const float* xp = x + plane * H * W;
    const float* yp = y + plane * H * W;
    const int tid = threadIdx.x;

    auto stage = [&](int lr, int lc, float xv, float yv) {
        const double ax = to01(xv, quantize_u8), ay = to01(yv, quantize_u8);
        sx[lr][lc] = (float)(ax - 0.5);
        sy[lr][lc] = (float)(ay - 0.5);
        if (lr < er && lc < ec) {               // owned pixel
            const double d = ax - ay;
            dsq[lr][lc] = d * d;
            dab[lr][lc] = fabs((double)xv - (double)yv);
        }
    };
    if (VEC) {
        constexpr int QW = RWP / 4;
        for (int t = tid; t < RH * QW; t += NT) {
            const int lr = t / QW, lc = (t % QW) * 4;
            const int64_t gr = r0 + lr, gc = c0 + lc;
            if (gr < H && gc < W) {             // W % 4 == 0 and c0 % 4 == 0: the whole float4 lies inside the row
                const float4 a = *reinterpret_cast<const float4*>(xp + gr * W + gc);
                const float4 b = *reinterpret_cast<const float4*>(yp + gr * W + gc);
                stage(lr, lc + 0, a.x, b.x);
                stage(lr, lc + 1, a.y, b.y);
                stage(lr, lc + 2, a.z, b.z);
                stage(lr, lc + 3, a.w, b.w);
            } else {
                *reinterpret_cast<float4*>(&sx[lr][lc]) = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(&sy[lr][lc]) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    } else {
        for (int t = tid; t < RH * RW; t += NT) {
            const int lr = t / RW, lc = t % RW;
            const int64_t gr = r0 + lr, gc = c0 + lc;
            if (gr < H && gc < W) {
                stage(lr, lc, xp[gr * W + gc], yp[gr * W + gc]);
            } else {
                sx[lr][lc] = 0.f;
                sy[lr][lc] = 0.f;
            }
        }
    }
    __syncthreads();
    // squared and absolute error: row segment of every piece, then the piece's rows top to bottom
    for (int t = tid; t < er * npc; t += NT) {
        const int i = t / npc, q = t % npc;
        const int j1 = min((q + 1) * pw, ec);
        double a = 0.0, b = 0.0;
        for (int j = q * pw; j < j1; ++j) {
            a += dsq[i][j];
            b += dab[i][j];
        }
        rp0[i][q] = a;
        rp1[i][q] = b;
    }
    __syncthreads();
    for (int t = tid; t < npr * npc; t += NT) {
        const int p = t / npc, q = t % npc;
        const int i1 = min((p + 1) * ph, er);
        double a = 0.0, b = 0.0;
        for (int i = p * ph; i < i1; ++i) {
            a += rp0[i][q];
            b += rp1[i][q];
        }
        out[(p * gm.c.cpt + q) * 3 + 0] = a;
        out[(p * gm.c.cpt + q) * 3 + 1] = b;
    }
    __syncthreads();                            // hp is about to hold the moments
    for (int t = tid; t < RH * TW; t += NT) {   // horizontal pass over every staged row
        const int r = t / TW, j = t % TW;
        float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float a = sx[r][j + k], b = sy[r][j + k], g = gw.g[k];
            mx += g * a;
            my += g * b;
            mxx += g * (a * a);
            myy += g * (b * b);
            mxy += g * (a * b);
        }
        hp[0][r][j] = mx;
        hp[1][r][j] = my;
        hp[2][r][j] = mxx;
        hp[3][r][j] = myy;
        hp[4][r][j] = mxy;
    }
    __syncthreads();                            // the staged images are free: the SSIM map takes their place
    const int64_t Ho = H - HALO, Wo = W - HALO;
    constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    for (int t = tid; t < TH * TW; t += NT) {   // vertical pass + the SSIM value of every owned valid window (0 elsewhere)
        const int i = t / TW, j = t % TW;
        float v = 0.f;
        if (i < er && j < ec && r0 + i < Ho && c0 + j < Wo) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float g = gw.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] += g * hp[q][i + k][j];
            }
            const float vx = m[2] - m[0] * m[0], vy = m[3] - m[1] * m[1], cxy = m[4] - m[0] * m[1];
            const float ux = m[0] + 0.5f, uy = m[1] + 0.5f;
            const float num = (2.f * ux * uy + C1) * (2.f * cxy + C2);
            const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
            v = num / den;
        }
        ssm[i][j] = v;
    }
    __syncthreads();                            // every read of hp is done: the row partials return to it
    for (int t = tid; t < er * npc; t += NT) {
        const int i = t / npc, q = t % npc;
        const int j1 = min((q + 1) * pw, ec);
        double a = 0.0;
        for (int j = q * pw; j < j1; ++j) a += (double)ssm[i][j];
        rp0[i][q] = a;
    }
    __syncthreads();
    for (int t = tid; t < npr * npc; t += NT) {
        const int p = t / npc, q = t % npc;
        const int i1 = min((p + 1) * ph, er);
        double a = 0.0;
        for (int i = p * ph; i < i1; ++i) a += rp0[i][q];
        out[(p * gm.c.cpt + q) * 3 + 2] = a;
    }
}

// one thread per (image, cell): its 3 * sub_r * sub_c slab entries, channel by channel, part by part
__global__ __launch_bounds__(NT) void recon_cells_fold_kernel(const double* __restrict__ slab, int64_t B, CellGeom gm,
                                                              double* __restrict__ cells) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int64_t ncell = (int64_t)gm.hg * gm.wg;
    if (e >= B * ncell) return;
    const int64_t b = e / ncell;
    const int gi = (int)((e % ncell) / gm.wg), gj = (int)(e % gm.wg);
    const int ppt = gm.r.cpt * gm.c.cpt;
    const int64_t ntiles = (int64_t)gm.r.ntile * gm.c.ntile;
    double a[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 3; ++c)
        for (int sr = 0; sr < gm.r.sub; ++sr)
            for (int sc = 0; sc < gm.c.sub; ++sc) {
                const int tr = gm.r.sub == 1 ? gi / gm.r.cpt : gi * gm.r.sub + sr;
                const int tc = gm.c.sub == 1 ? gj / gm.c.cpt : gj * gm.c.sub + sc;
                const int p = gm.r.sub == 1 ? gi % gm.r.cpt : 0, q = gm.c.sub == 1 ? gj % gm.c.cpt : 0;
                const double* s = slab + (((b * 3 + c) * ntiles + (int64_t)tr * gm.c.ntile + tc) * ppt + p * gm.c.cpt + q) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) a[k] += s[k];
            }
#pragma unroll
    for (int k = 0; k < 3; ++k) cells[e * 3 + k] = a[k];
}

__global__ __launch_bounds__(NT) void code_histogram_kernel(const int64_t* __restrict__ idx, const int64_t* __restrict__ grain,
                                                            int64_t Hf, int64_t Wf, int64_t hg, int64_t wg, int64_t r, int64_t K,
                                                            int G, int64_t* __restrict__ counts, int64_t* __restrict__ tokens,
                                                            int64_t* __restrict__ invalid) {
    __shared__ long long red[NT / DVQ_WAVE][2];
    const int64_t b = blockIdx.x;
    const int64_t* ib = idx + b * Hf * Wf;
    const int64_t* gb = grain ? grain + b * hg * wg : nullptr;
    long long cnt = 0, bad = 0;
    for (int64_t p = threadIdx.x; p < Hf * Wf; p += NT) {
        const int64_t i = p / Wf, j = p % Wf;
        int64_t g = 0, s = 1;
        if (gb) {
            g = gb[(i / r) * wg + j / r];
            if (g < 0 || g >= G) {              // an invalid grain value counts once per grain cell, and the cell gives no tokens
                if (i % r == 0 && j % r == 0) ++bad;
                continue;
            }
            s = r >> g;                         // token stride inside the cell: the coarsest grain spends one token per cell
        }
        if (i % s != 0 || j % s != 0) continue;
        ++cnt;
        const int64_t code = ib[p];
        if (code < 0 || code >= K) {
            ++bad;
            continue;
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(counts + g * K + code), 1ull);
    }
    cnt = wave_sum(cnt);
    bad = wave_sum(bad);
    const int wid = threadIdx.x / DVQ_WAVE;
    if ((threadIdx.x % DVQ_WAVE) == 0) {
        red[wid][0] = cnt;
        red[wid][1] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long c = 0, e = 0;
#pragma unroll
        for (int w = 0; w < NT / DVQ_WAVE; ++w) {
            c += red[w][0];
            e += red[w][1];
        }
        tokens[b] = c;
        if (e) atomicAdd(reinterpret_cast<unsigned long long*>(invalid), (unsigned long long)e);
    }
}

Gauss11 gaussian11() {
    double w[11], s = 0.0;
    for (int k = 0; k < 11; ++k) {
        const double d = k - 5;
        w[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        s += w[k];
    }
    Gauss11 g;
    for (int k = 0; k < 11; ++k) g.g[k] = (float)(w[k] / s);
    return g;
}

void tile_grid(int64_t H, int64_t W, int64_t* tiles_x, int64_t* ntiles) {
    *tiles_x = cdiv64(W, TW);
    *ntiles = cdiv64(H, TH) * *tiles_x;
}

CellAxis cell_axis(int64_t n_pix, int64_t n_cells, int T) {
    CellAxis a;
    a.cell = (int)(n_pix / n_cells);
    if (a.cell <= T) {
        a.cpt = T / a.cell;
        a.sub = 1;
        a.ntile = (int)cdiv64(n_cells, a.cpt);
    } else {
        a.cpt = 1;
        a.sub = (int)cdiv64(a.cell, T);
        a.ntile = (int)(n_cells * a.sub);
    }
    return a;
}

bool cell_grid_ok(int64_t B, int64_t H, int64_t W, int64_t hg, int64_t wg) {
    return B > 0 && H > 0 && W > 0 && hg > 0 && wg > 0 && H < (1ll << 24) && W < (1ll << 24) && H % hg == 0 && W % wg == 0;
}

CellGeom cell_geom(int64_t H, int64_t W, int64_t hg, int64_t wg) {
    CellGeom g;
    g.r = cell_axis(H, hg, TH);
    g.c = cell_axis(W, wg, TW);
    g.hg = (int)hg;
    g.wg = (int)wg;
    return g;
}

}  // namespace

extern "C" size_t dvq_recon_cells_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t hg, int64_t wg) {
    if (!cell_grid_ok(B, H, W, hg, wg)) return 0;
    const CellGeom g = cell_geom(H, W, hg, wg);
    return (size_t)B * 3 * (size_t)g.r.ntile * g.c.ntile * (size_t)(g.r.cpt * g.c.cpt) * 3 * sizeof(double);
}

extern "C" int dvq_recon_cells(const float* x, const float* y, int64_t B, int64_t H, int64_t W, int64_t hg, int64_t wg, int quantize_u8,
                               double* cells, void* ws, size_t ws_bytes, dvq_stream_t stream) {
    DVQ_REQUIRE(x && y && cells && ws, DVQ_EINVAL, "dvq_recon_cells: null pointer");
    DVQ_REQUIRE(quantize_u8 == 0 || quantize_u8 == 1, DVQ_EINVAL, "dvq_recon_cells: quantize_u8=%d is not 0 or 1", quantize_u8);
    DVQ_REQUIRE(cell_grid_ok(B, H, W, hg, wg), DVQ_ESHAPE,
                "dvq_recon_cells: B=%lld H=%lld W=%lld over a %lld x %lld cell grid (H %% hg == 0 and W %% wg == 0 are needed)",
                (long long)B, (long long)H, (long long)W, (long long)hg, (long long)wg);
    const CellGeom g = cell_geom(H, W, hg, wg);
    const size_t need = dvq_recon_cells_workspace_bytes(B, H, W, hg, wg);
    DVQ_REQUIRE(ws_bytes >= need, DVQ_EWORKSPACE, "dvq_recon_cells: workspace %zu bytes < %zu", ws_bytes, need);
    const int64_t nblk = B * 3 * g.r.ntile * g.c.ntile, ncell = B * hg * wg;
    DVQ_REQUIRE(nblk < (1ll << 31) && ncell < (1ll << 31), DVQ_ESHAPE, "dvq_recon_cells: %lld tiles / %lld cells is too many",
                (long long)nblk, (long long)ncell);
    hipStream_t s = (hipStream_t)stream;
    double* slab = static_cast<double*>(ws);
    const Gauss11 gw = gaussian11();
    // 16-byte loads need every tile origin on a multiple of 4 columns: W % 4 == 0 and a cell width that is one
    const bool vec = W % 4 == 0 && g.c.cell % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    if (vec)
        recon_cells_tile_kernel<true><<<dim3((unsigned)nblk), dim3(NT), 0, s>>>(x, y, H, W, g, quantize_u8, gw, slab);
    else
        recon_cells_tile_kernel<false><<<dim3((unsigned)nblk), dim3(NT), 0, s>>>(x, y, H, W, g, quantize_u8, gw, slab);
    DVQ_CHECK_LAUNCH("recon_cells_tile");
    recon_cells_fold_kernel<<<dim3((unsigned)cdiv64(ncell, NT)), dim3(NT), 0, s>>>(slab, B, g, cells);
    DVQ_CHECK_LAUNCH("recon_cells_fold");
    return DVQ_OK;
}

extern "C" size_t dvq_recon_metrics_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    int64_t tx, nt;
    tile_grid(H, W, &tx, &nt);
    return (size_t)B * 3 * (size_t)nt * 3 * sizeof(double);
}

extern "C" int dvq_recon_metrics(const float* x, const float* y, int64_t B, int64_t H, int64_t W, int quantize_u8, double* mse,
                                 double* l1, double* ssim, void* ws, size_t ws_bytes, dvq_stream_t stream) {
    DVQ_REQUIRE(x && y && mse && l1 && ssim && ws, DVQ_EINVAL, "dvq_recon_metrics: null pointer");
    DVQ_REQUIRE(quantize_u8 == 0 || quantize_u8 == 1, DVQ_EINVAL, "dvq_recon_metrics: quantize_u8=%d is not 0 or 1", quantize_u8);
    DVQ_REQUIRE(B > 0 && H >= 11 && W >= 11, DVQ_ESHAPE,
                "dvq_recon_metrics: B=%lld H=%lld W=%lld (SSIM needs H, W >= 11: the 11 x 11 window's valid region is empty)",
                (long long)B, (long long)H, (long long)W);
    int64_t tx, nt;
    tile_grid(H, W, &tx, &nt);
    const size_t need = dvq_recon_metrics_workspace_bytes(B, H, W);
    DVQ_REQUIRE(ws_bytes >= need, DVQ_EWORKSPACE, "dvq_recon_metrics: workspace %zu bytes < %zu", ws_bytes, need);
    const int64_t nblk = B * 3 * nt;
    DVQ_REQUIRE(nblk < (1ll << 31) && nt < (1ll << 30), DVQ_ESHAPE, "dvq_recon_metrics: %lld tiles is too many", (long long)nblk);
    hipStream_t s = (hipStream_t)stream;
    double* slab = static_cast<double*>(ws);
    const Gauss11 g = gaussian11();
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    if (vec)
        recon_metrics_tile_kernel<true><<<dim3((unsigned)nblk), dim3(NT), 0, s>>>(x, y, H, W, (int)tx, (int)nt, quantize_u8, g, slab);
    else
        recon_metrics_tile_kernel<false><<<dim3((unsigned)nblk), dim3(NT), 0, s>>>(x, y, H, W, (int)tx, (int)nt, quantize_u8, g, slab);
    DVQ_CHECK_LAUNCH("recon_metrics_tile");
    const double inv_pix = 1.0 / (3.0 * (double)H * (double)W);
    const double inv_pos = 1.0 / (3.0 * (double)(H - HALO) * (double)(W - HALO));
    recon_metrics_fold_kernel<<<dim3((unsigned)B), dim3(DVQ_WAVE), 0, s>>>(slab, 3 * nt, inv_pix, inv_pos, mse, l1, ssim);
    DVQ_CHECK_LAUNCH("recon_metrics_fold");
    return DVQ_OK;
}

extern "C" int dvq_code_histogram(const int64_t* idx, const int64_t* grain, int64_t B, int64_t Hf, int64_t Wf, int64_t hg, int64_t wg,
                                  int64_t K, int G, int64_t* counts, int64_t* tokens, int64_t* invalid, dvq_stream_t stream) {
    DVQ_REQUIRE(idx && counts && tokens && invalid, DVQ_EINVAL, "dvq_code_histogram: null pointer");
    DVQ_REQUIRE(K > 0 && G >= 1 && G <= 3, DVQ_EINVAL, "dvq_code_histogram: K=%lld G=%d (K > 0, G in 1..3)", (long long)K, G);
    DVQ_REQUIRE(B > 0 && B < (1ll << 31) && Hf > 0 && Wf > 0, DVQ_ESHAPE, "dvq_code_histogram: bad code map shape");
    int64_t r = 1;
    if (grain) {
        DVQ_REQUIRE(hg > 0 && wg > 0 && Hf % hg == 0 && Wf % wg == 0 && Hf / hg == Wf / wg && Hf / hg == (1ll << (G - 1)), DVQ_ESHAPE,
                    "dvq_code_histogram: code map %lld x %lld over grain map %lld x %lld needs a cell of 2^(G-1) = %lld codes per side",
                    (long long)Hf, (long long)Wf, (long long)hg, (long long)wg, 1ll << (G - 1));
        r = Hf / hg;
    } else {
        DVQ_REQUIRE(G == 1, DVQ_ESHAPE, "dvq_code_histogram: G=%d needs a grain map", G);
    }
    code_histogram_kernel<<<dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream>>>(idx, grain, Hf, Wf, hg, wg, r, K, G, counts, tokens,
                                                                                   invalid);
    DVQ_CHECK_LAUNCH("code_histogram");
    return DVQ_OK;
}
