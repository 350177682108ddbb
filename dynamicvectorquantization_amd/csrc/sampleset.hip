// Sample-set metrics on feature vectors (gfx950): the all-pairs scan behind improved precision / recall (Kynkaanniemi et al. 2019) and
// density / coverage (Naeem et al. 2020), and the moments behind the Frechet distance.  No counterpart in the reference: its samplers
// stop at an .npz "for an external tool".  docs/design/32-sample-set-metrics.md has the definitions and the accuracy derivation.
//
// dvq_pair_scan: one workgroup (4 waves) per 128 rows of a and per split of b's 128-row tiles.  Per tile pair the inner products run on
// v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation: a k-ordered fmaf chain), each wave holding 2 x 2 accumulator tiles
// of 32 x 32; the operands are staged through LDS in 32-column chunks, the next chunk's global loads in flight while the current one
// is multiplied.  Row norms are summed in fp64 from the staged chunks (exact products) and rounded once to fp32.  The distances of a
// tile pair never leave the workgroup: they are written to LDS (over the free staging area, 64 columns at a time) and ONE thread per
// row of a walks them in ascending j, counting d2 <= rad2_b[j] and keeping its k best in a sorted list in LDS (strict `<` against
// the current k-th, insertion behind equal values: ties go to the lower index).  With several splits the lists go to the workspace
// and a second kernel merges them per row in split order.  No float atomics; every output has one owner.
// The value of d2(i, j) depends on row i of a, row j of b and D only (one fmaf chain per block of 64 columns, within every 8 columns
// in the order 0, 4, 1, 5, 2, 6, 3, 7, the block sums added in order; zero padding adds exact zeros), and (d2, j) is a total order: neither the tile a row falls into nor the number of splits can change
// a result bit.
// dvq_feat_moments: one workgroup per 64 x 64 tile of the upper triangle of the Gram matrix; a thread owns 4 x 4 entries and walks the
// rows in order with fp64 FMAs on exact products (y = fl32(x - shift) staged in LDS, 32 rows at a time).  Diagonal tiles also own
// the column sums.  Plain FMAs, not the fp64 MFMA: at D = 1024 and N = 50 000 the pass is 0.05 TFLOP next to four scans of 5 TFLOP.
#include "dvq_common.h"

#include <math.h>

namespace {

constexpr int PT = 128;                 // rows of a, and of b, per tile
constexpr int PKC = 32;                 // feature columns per staged chunk
constexpr int PFOLD = 2;                // chunks per summation block: the fmaf chain restarts every 64 columns
constexpr int PLD = PKC + 4;            // LDS row stride of a staged chunk: 16-B aligned rows, conflict-free 16-B reads down a column
constexpr int PNT = 256;
constexpr int PDH = 64;                 // b columns of the distance tile per selection pass
constexpr int PDLD = PDH + 1;
constexpr int PKMAX = 16;
constexpr int PKLD = PKMAX + 1;
constexpr int PMAXSPLIT = 16;
constexpr int PTARGET_BLOCKS = 512;     // two resident workgroups on each of 256 CUs

struct PairArgs {
    const float* a;
    const float* b;
    const float* rad2;
    int64_t Na, Nb, D, lda, ldb;
    int k, exclude_diag, splits, tiles_per_split;
    float* kth2;            // outputs (written directly when splits == 1)
    int64_t* idx;
    int64_t* count;
    int64_t* pc;            // per-split partials [splits][Na], [splits][Na][k], [splits][Na][k]
    float* pd;
    int* pi;
};

// rows [row0, row0 + 128) x columns [kk, kk + 32) of m (nrows rows of pitch ld, D used columns) -> 4 float4 per thread; rows past
// nrows and columns past D read as 0 and are never touched in memory
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float* __restrict__ m, int64_t ld, int64_t row0, int64_t nrows, int64_t D, int64_t kk,
                                           int tid, float4 (&v)[4]) {
    const int64_t c = kk + (tid & 7) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = row0 + (tid >> 3) + 32 * q;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nrows && c < D) {
            const float* p = m + r * ld + c;
            if (VEC && c + 4 <= D) {
                t = *reinterpret_cast<const float4*>(p);
            } else {
                t.x = p[0];
                if (c + 1 < D) t.y = p[1];
                if (c + 2 < D) t.z = p[2];
                if (c + 3 < D) t.w = p[3];
            }
        }
        v[q] = t;
    }
}

__device__ __forceinline__ void store_chunk(float* __restrict__ s, int tid, const float4 (&v)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(s + ((tid >> 3) + 32 * q) * PLD + (tid & 7) * 4) = v[q];
}

template <bool VEC>
__global__ __launch_bounds__(PNT, 2) void pair_scan_kernel(PairArgs p) {
    __shared__ __attribute__((aligned(16))) float stage[2 * PT * PLD];      // a chunk | b chunk; between tiles: the distance tile
    __shared__ float sna[PT], snb[PT], srad[PT];
    __shared__ float kd[PT][PKLD];
    __shared__ int ki[PT][PKLD];
    static_assert(PT * PDLD <= 2 * PT * PLD, "the distance tile shares the staging area");
    float* As = stage;
    float* Bs = stage + PT * PLD;
    float* dist = stage;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;                    // the wave's 64 x 64 quarter of the 128 x 128 tile pair
    const int64_t i0 = (int64_t)blockIdx.x * PT;
    const int split = blockIdx.y;
    const int64_t ntiles = (p.Nb + PT - 1) / PT;
    const int64_t t_begin = (int64_t)split * p.tiles_per_split;
    const int64_t t_end = min(t_begin + p.tiles_per_split, ntiles);
    const int k = p.k;
    const int64_t nchunks = (p.D + PKC - 1) / PKC;
    const float inf = __builtin_inff();

    if (tid < PT)
        for (int q = 0; q < k; ++q) {
            kd[tid][q] = inf;
            ki[tid][q] = -1;
        }
    long long cnt = 0;
    float thr = inf;                                            // the owner's current k-th distance
    const int64_t irow = i0 + tid;                              // row of a this thread owns (tid < PT)

    for (int64_t jt = t_begin; jt < t_end; ++jt) {
        const int64_t j0 = jt * PT;
        const bool first = jt == t_begin;
        f32x16 acc[2][2], tot[2][2];                            // the running 64-column block, and the sum of the blocks before it
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = tot[mt][nt][r] = 0.f;
        double n64 = 0.0;                                       // |row|^2: threads 0..127 a's rows (first tile only), 128..255 b's rows
        float4 ra[4], rb[4];
        load_chunk<VEC>(p.a, p.lda, i0, p.Na, p.D, 0, tid, ra);
        load_chunk<VEC>(p.b, p.ldb, j0, p.Nb, p.D, 0, tid, rb);
        for (int64_t c = 0; c < nchunks; ++c) {
            store_chunk(As, tid, ra);
            store_chunk(Bs, tid, rb);
            __syncthreads();
            if (c + 1 < nchunks) {
                load_chunk<VEC>(p.a, p.lda, i0, p.Na, p.D, (c + 1) * PKC, tid, ra);
                load_chunk<VEC>(p.b, p.ldb, j0, p.Nb, p.D, (c + 1) * PKC, tid, rb);
            }
#pragma unroll
            for (int s = 0; s < PKC / 8; ++s) {
                float4 av[2], bv[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    av[t] = *reinterpret_cast<const float4*>(As + (wm * 64 + t * 32 + (lane & 31)) * PLD + s * 8 + 4 * (lane >> 5));
                    bv[t] = *reinterpret_cast<const float4*>(Bs + (wn * 64 + t * 32 + (lane & 31)) * PLD + s * 8 + 4 * (lane >> 5));
                }
                const float a4[2][4] = {{av[0].x, av[0].y, av[0].z, av[0].w}, {av[1].x, av[1].y, av[1].z, av[1].w}};
                const float b4[2][4] = {{bv[0].x, bv[0].y, bv[0].z, bv[0].w}, {bv[1].x, bv[1].y, bv[1].z, bv[1].w}};
#pragma unroll
                for (int q = 0; q < 4; ++q)                     // instruction q multiplies columns 8s + q (lanes 0..31) and 8s + 4 + q
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[mt][q], b4[nt][q], acc[mt][nt], 0, 0, 0);
            }
            if ((c & (PFOLD - 1)) == PFOLD - 1 || c + 1 == nchunks) {
                // blocked summation: a chain of 1024 fmaf carries ~4 x the rounding error of 16 chains of 64 and their sum
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            tot[mt][nt][r] += acc[mt][nt][r];
                            acc[mt][nt][r] = 0.f;
                        }
            }
            if (tid >= PT || first) {
                const float* row = (tid < PT ? As : Bs) + (tid & (PT - 1)) * PLD;
#pragma unroll
                for (int q = 0; q < PKC / 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4*>(row + 4 * q);
                    n64 = fma((double)v.x, (double)v.x, n64);
                    n64 = fma((double)v.y, (double)v.y, n64);
                    n64 = fma((double)v.z, (double)v.z, n64);
                    n64 = fma((double)v.w, (double)v.w, n64);
                }
            }
            __syncthreads();
        }
        if (tid < PT) {
            if (first) sna[tid] = (float)n64;
        } else {
            const int64_t j = j0 + tid - PT;
            snb[tid - PT] = (float)n64;
            srad[tid - PT] = (p.rad2 != nullptr && j < p.Nb) ? p.rad2[j] : -1.f;
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (wn == pass) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                            const int col = nt * 32 + (lane & 31);
                            const float d = fmaf(-2.f, tot[mt][nt][r], sna[row] + snb[pass * PDH + col]);
                            dist[row * PDLD + col] = d < 0.f ? 0.f : d;         // a NaN stays a NaN: it is never selected or counted
                        }
            }
            __syncthreads();
            if (tid < PT && irow < p.Na) {
                for (int c = 0; c < PDH; ++c) {
                    const int64_t j = j0 + pass * PDH + c;
                    if (j >= p.Nb) break;
                    if (p.exclude_diag && j == irow) continue;
                    const float d = dist[tid * PDLD + c];
                    cnt += d <= srad[pass * PDH + c] ? 1 : 0;
                    if (d < thr) {
                        int pos = k - 1;
                        while (pos > 0 && kd[tid][pos - 1] > d) {
                            kd[tid][pos] = kd[tid][pos - 1];
                            ki[tid][pos] = ki[tid][pos - 1];
                            --pos;
                        }
                        kd[tid][pos] = d;
                        ki[tid][pos] = (int)j;
                        thr = kd[tid][k - 1];
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid < PT && irow < p.Na) {
        if (p.splits == 1) {
            for (int q = 0; q < k; ++q) {
                p.kth2[irow * k + q] = kd[tid][q];
                p.idx[irow * k + q] = (int64_t)ki[tid][q];
            }
            if (p.rad2 != nullptr) p.count[irow] = cnt;
        } else {
            const int64_t e = (int64_t)split * p.Na + irow;
            for (int q = 0; q < k; ++q) {
                p.pd[e * k + q] = kd[tid][q];
                p.pi[e * k + q] = ki[tid][q];
            }
            p.pc[e] = cnt;
        }
    }
}

// one thread per row of a: its `splits` sorted lists, lower split first on equal distances (a lower split holds lower j)
__global__ __launch_bounds__(PNT) void pair_merge_kernel(PairArgs p) {
    const int64_t i = (int64_t)blockIdx.x * PNT + threadIdx.x;
    if (i >= p.Na) return;
    const int k = p.k;
    int head[PMAXSPLIT];
#pragma unroll
    for (int s = 0; s < PMAXSPLIT; ++s) head[s] = 0;
    for (int q = 0; q < k; ++q) {
        int best = -1, bi = -1;
        float bd = __builtin_inff();
#pragma unroll
        for (int s = 0; s < PMAXSPLIT; ++s) {
            if (s < p.splits && head[s] < k) {
                const int64_t e = ((int64_t)s * p.Na + i) * k + head[s];
                const int ji = p.pi[e];
                const float d = p.pd[e];
                if (ji >= 0 && (best < 0 || d < bd)) {
                    best = s;
                    bd = d;
                    bi = ji;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < PMAXSPLIT; ++s)
            if (s == best) ++head[s];
        p.kth2[i * k + q] = bd;
        p.idx[i * k + q] = (int64_t)bi;
    }
    if (p.rad2 != nullptr) {
        long long c = 0;
        for (int s = 0; s < p.splits; ++s) c += p.pc[(int64_t)s * p.Na + i];
        p.count[i] = c;
    }
}

bool pair_shape_ok(int64_t Na, int64_t Nb, int k) {
    return Na > 0 && Nb > 0 && Nb < (1ll << 31) && Na < (1ll << 37) && k >= 1 && k <= PKMAX;
}

// how b's tiles are shared out: enough workgroups to fill the chip when a has few rows, never an empty split
int pair_splits(int64_t Na, int64_t Nb, int* tiles_per_split) {
    const int64_t nba = cdiv64(Na, PT), ntiles = cdiv64(Nb, PT);
    int64_t want = PTARGET_BLOCKS / nba;
    want = want < 1 ? 1 : want;
    want = want > PMAXSPLIT ? PMAXSPLIT : want;
    want = want > ntiles ? ntiles : want;
    const int64_t tps = cdiv64(ntiles, want);
    *tiles_per_split = (int)tps;
    return (int)cdiv64(ntiles, tps);
}

// ---- moments -----------------------------------------------------------------------------------------------------------------------
constexpr int MT = 64;                  // Gram tile edge
constexpr int MNB = 32;                 // rows staged per step

__global__ __launch_bounds__(PNT) void feat_moments_kernel(const float* __restrict__ x, int64_t N, int64_t D, int64_t ld,
                                                           const float* __restrict__ shift, double* __restrict__ sum,
                                                           double* __restrict__ gram, int64_t* __restrict__ n) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;                                        // upper triangle only
    __shared__ __attribute__((aligned(16))) float yi[MNB][MT];
    __shared__ __attribute__((aligned(16))) float yj[MNB][MT];
    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;                     // owner of rows ty * 4 .. + 3 (tile ti), columns tx * 4 .. + 3 (tile tj)
    const int lc = tid & 63;
    const int64_t ci = (int64_t)ti * MT + lc, cj = (int64_t)tj * MT + lc;
    const float shi = ci < D ? shift[ci] : 0.f, shj = cj < D ? shift[cj] : 0.f;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    double csum = 0.0;
    for (int64_t n0 = 0; n0 < N; n0 += MNB) {
#pragma unroll
        for (int q = 0; q < MNB / 4; ++q) {
            const int r = (tid >> 6) + 4 * q;
            const int64_t row = n0 + r;
            float vi = 0.f, vj = 0.f;
            if (row < N) {
                if (ci < D) vi = x[row * ld + ci] - shi;
                if (cj < D) vj = x[row * ld + cj] - shj;
            }
            yi[r][lc] = vi;
            yj[r][lc] = vj;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < MNB; ++r) {
            const float4 a = *reinterpret_cast<const float4*>(&yi[r][ty * 4]);
            const float4 b = *reinterpret_cast<const float4*>(&yj[r][tx * 4]);
            const double ad[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
            const double bd[4] = {(double)b.x, (double)b.y, (double)b.z, (double)b.w};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(ad[u], bd[v], acc[u][v]);
        }
        if (ti == tj && tid < MT)
            for (int r = 0; r < MNB; ++r) csum += (double)yi[r][tid];
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t gi = (int64_t)ti * MT + ty * 4 + u, gj = (int64_t)tj * MT + tx * 4 + v;
            if (gi < D && gj < D && gi <= gj) gram[gi * D + gj] += acc[u][v];
        }
    if (ti == tj && tid < MT && ci < D) sum[ci] += csum;
    if (ti == 0 && tj == 0 && tid == 0) n[0] += N;
}

}  // namespace

extern "C" size_t dvq_pair_scan_workspace_bytes(int64_t Na, int64_t Nb, int k) {
    if (!pair_shape_ok(Na, Nb, k)) return 0;
    int tps;
    const int splits = pair_splits(Na, Nb, &tps);
    if (splits == 1) return 0;
    return (size_t)splits * (size_t)Na * ((size_t)k * (sizeof(float) + sizeof(int)) + sizeof(int64_t));
}

extern "C" int dvq_pair_scan(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t Na, int64_t Nb, int64_t D,
                             const float* rad2_b, int k, int exclude_diag, float* kth2, int64_t* idx, int64_t* count, void* ws,
                             size_t ws_bytes, dvq_stream_t stream) {
    DVQ_REQUIRE(a && b && kth2 && idx && (rad2_b == nullptr || count != nullptr), DVQ_EINVAL, "dvq_pair_scan: null pointer");
    DVQ_REQUIRE(k >= 1 && k <= PKMAX, DVQ_EINVAL, "dvq_pair_scan: k=%d is not in [1, %d]", k, PKMAX);
    DVQ_REQUIRE(exclude_diag == 0 || exclude_diag == 1, DVQ_EINVAL, "dvq_pair_scan: exclude_diag=%d is not 0 or 1", exclude_diag);
    DVQ_REQUIRE(pair_shape_ok(Na, Nb, k) && D >= 1 && D <= (1ll << 24) && lda >= D && ldb >= D, DVQ_ESHAPE,
                "dvq_pair_scan: Na=%lld Nb=%lld D=%lld lda=%lld ldb=%lld (Na, Nb, D >= 1, Nb < 2^31, pitches >= D)", (long long)Na,
                (long long)Nb, (long long)D, (long long)lda, (long long)ldb);
    PairArgs p;
    p.a = a;
    p.b = b;
    p.rad2 = rad2_b;
    p.Na = Na;
    p.Nb = Nb;
    p.D = D;
    p.lda = lda;
    p.ldb = ldb;
    p.k = k;
    p.exclude_diag = exclude_diag;
    p.splits = pair_splits(Na, Nb, &p.tiles_per_split);
    p.kth2 = kth2;
    p.idx = idx;
    p.count = count;
    p.pc = nullptr;
    p.pd = nullptr;
    p.pi = nullptr;
    if (p.splits > 1) {
        const size_t need = dvq_pair_scan_workspace_bytes(Na, Nb, k);
        DVQ_REQUIRE(ws != nullptr && ws_bytes >= need, DVQ_EWORKSPACE, "dvq_pair_scan: workspace %zu bytes < %zu", ws ? ws_bytes : (size_t)0,
                    need);
        DVQ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, DVQ_EINVAL, "dvq_pair_scan: the workspace is not 8-byte aligned");
        const size_t rows = (size_t)p.splits * (size_t)Na;
        p.pc = static_cast<int64_t*>(ws);
        p.pd = reinterpret_cast<float*>(p.pc + rows);
        p.pi = reinterpret_cast<int*>(p.pd + rows * (size_t)k);
    }
    const int64_t nba = cdiv64(Na, PT);
    DVQ_REQUIRE(nba < (1ll << 31), DVQ_ESHAPE, "dvq_pair_scan: %lld row tiles is too many", (long long)nba);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = lda % 4 == 0 && ldb % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0;
    const dim3 grid((unsigned)nba, (unsigned)p.splits);
    if (vec)
        pair_scan_kernel<true><<<grid, dim3(PNT), 0, s>>>(p);
    else
        pair_scan_kernel<false><<<grid, dim3(PNT), 0, s>>>(p);
    DVQ_CHECK_LAUNCH("pair_scan");
    if (p.splits > 1) {
        pair_merge_kernel<<<dim3((unsigned)cdiv64(Na, PNT)), dim3(PNT), 0, s>>>(p);
        DVQ_CHECK_LAUNCH("pair_merge");
    }
    return DVQ_OK;
}

extern "C" int dvq_feat_moments(const float* x, int64_t N, int64_t D, int64_t ld, const float* shift, double* sum, double* gram,
                                int64_t* n, dvq_stream_t stream) {
    DVQ_REQUIRE(x && shift && sum && gram && n, DVQ_EINVAL, "dvq_feat_moments: null pointer");
    DVQ_REQUIRE(N >= 1 && D >= 1 && D <= 4096 && ld >= D, DVQ_ESHAPE, "dvq_feat_moments: N=%lld D=%lld ld=%lld (N >= 1, D in [1, 4096], ld >= D)",
                (long long)N, (long long)D, (long long)ld);
    const unsigned t = (unsigned)cdiv64(D, MT);
    feat_moments_kernel<<<dim3(t, t), dim3(PNT), 0, (hipStream_t)stream>>>(x, N, D, ld, shift, sum, gram, n);
    DVQ_CHECK_LAUNCH("feat_moments");
    return DVQ_OK;
}
