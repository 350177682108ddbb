"""numpy restatements of the sample-set metrics (docs/design/32-sample-set-metrics.md): the all-pairs scan in fp64 and in the kernel's
fp32 staging, the moments, the Frechet distance and the five set metrics -- no GPU, no torch.  tests/test_sampleset_cpu.py checks
them against brute-force definitions; tests/test_gpu_sampleset.py holds the kernels to them."""
import numpy as np

# the pair_scan shape matrix: (Na, Nb, D, k).  The first six are the issue's; the others are the kernel's own edges, each with its reason
PAIR_CASES = [
    (80, 96, 24, 3),
    (64, 65, 7, 1),
    (33, 130, 256, 5),
    (257, 300, 1000, 5),
    (300, 257, 1024, 3),
    (40, 40, 3, 16),
]
PAIR_EDGE_CASES = [
    (128, 128, 32, 4),      # exactly one 128 x 128 tile pair and one 32-column chunk: no padding row, column or chunk anywhere
    (129, 129, 33, 4),      # one past each: a second row tile, a second b tile (so b is split in two) and a second chunk, all but empty
    (20, 256, 36, 2),       # b of exactly two tiles: split in two, each split one full tile; pitch % 4 == 0 with D % 32 != 0
    (20, 2100, 12, 16),     # 17 tiles of b: more tiles than the 16 splits allowed, so splits hold two tiles (the last: one); k = 16 merge
]
BAND = 1e-5                 # decisions closer than BAND * (|a|^2 + |b|^2) to their threshold are not held exactly
# worst deviation of d2_f32_staged from d2_fp64 over the ten cases above (real | fake | real-real scans of make_sets at case_seed), in
# units of |a|^2 + |b|^2, measured on the CPU (tests/test_sampleset_cpu.py re-measures it); the GPU is granted 4 x: another device's
# fma and the rare double rounding of the restated one
STAGING_YARDSTICK = 3.6e-7
GRANTED = 4 * STAGING_YARDSTICK


def case_seed(na, nb, d):
    return na * 7 + d


def make_sets(n_real, n_fake, d, seed):
    """low-dimensional structure in D dimensions (isotropic Gaussians make every distance the same and every metric degenerate):
    rows = z W + 0.05 noise + 1.5 with z ~ N(0, I_q), q = min(6, D), W ~ N(0, 1/6); the fake set uses 0.9 z, + 0.4 on latent axis 0"""
    rng = np.random.default_rng(seed)
    q = min(6, d)
    w = rng.normal(0.0, np.sqrt(1.0 / 6.0), size=(q, d))
    zr = rng.normal(size=(n_real, q))
    zf = 0.9 * rng.normal(size=(n_fake, q))
    zf[:, 0] += 0.4
    real = zr @ w + 0.05 * rng.normal(size=(n_real, d)) + 1.5
    fake = zf @ w + 0.05 * rng.normal(size=(n_fake, d)) + 1.5
    return real, fake


def centre(real, fake):
    """both sets minus the REAL set's fp64 mean, cast to fp32: what every scan and moment pass sees"""
    mean = np.asarray(real, np.float64).mean(axis=0)
    return (np.asarray(real, np.float64) - mean).astype(np.float32), (np.asarray(fake, np.float64) - mean).astype(np.float32)


def d2_fp64(a, b):
    """sum_c (a_ic - b_jc)^2 in fp64, the difference form (no cancellation)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    for i in range(a.shape[0]):
        out[i] = ((b - a[i]) ** 2).sum(axis=1)
    return out


def norm_scale(a, b):
    """|a_i|^2 + |b_j|^2 in fp64: the unit of the GEMM form's error"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :]


K_ORDER = (0, 4, 1, 5, 2, 6, 3, 7)      # the order the matrix instruction meets the columns of a group of 8
K_BLOCK = 64                            # columns per fma chain: the chain restarts every 64 columns and the block sums are added in order


def d2_f32_staged(a, b):
    """the kernel's arithmetic restated in numpy float32: norms summed in fp64 from exact squares and rounded once; the inner product
    one fp32 fused-multiply-add chain per pair and block of 64 columns in the kernel's column order, the block sums added in order (the fma as: exact fp64 product + fp64 sum, rounded to
    fp32); d2 = max(fl32(fl32(na + nb) - 2 dot), 0)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = a.shape[1]
    na = (a.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    nb = (b.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dot = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for blk in range(0, d, K_BLOCK):
        part = np.zeros_like(dot)
        for g in range(blk, min(blk + K_BLOCK, d), 8):
            for o in K_ORDER:
                c = g + o
                if c < d:
                    part = (part.astype(np.float64) + a64[:, c, None] * b64[None, :, c]).astype(np.float32)
        dot = dot + part
    s = (na[:, None] + nb[None, :]).astype(np.float32)
    return np.maximum((s - np.float32(2.0) * dot).astype(np.float32), np.float32(0.0))


def staging_error(a, b):
    """worst |d2_f32_staged - d2_fp64| / (|a|^2 + |b|^2) over all pairs"""
    return float(np.max(np.abs(d2_f32_staged(a, b).astype(np.float64) - d2_fp64(a, b)) / np.maximum(norm_scale(a, b), 1e-300)))


def pair_scan_ref(a, b, k, rad2_b=None, exclude_diag=False, d2=None):
    """-> (kth2 [Na, k] ascending, +inf padded; idx int64 [Na, k], -1 padded, lower index first on equal distances; count int64 [Na]
    or None) from the fp64 distances (or from `d2`)"""
    d2 = d2_fp64(a, b) if d2 is None else np.array(d2, dtype=np.float64)
    na, nb = d2.shape
    valid = np.ones((na, nb), bool)
    if exclude_diag:
        valid[np.arange(min(na, nb)), np.arange(min(na, nb))] = False
    kth2 = np.full((na, k), np.inf)
    idx = np.full((na, k), -1, np.int64)
    for i in range(na):
        js = np.flatnonzero(valid[i])
        order = js[np.argsort(d2[i, js], kind="stable")][:k]
        kth2[i, :order.size] = d2[i, order]
        idx[i, :order.size] = order
    count = None
    if rad2_b is not None:
        count = ((d2 <= np.asarray(rad2_b, np.float64)[None, :]) & valid).sum(axis=1).astype(np.int64)
    return kth2, idx, count


def in_band(d2, rad2_b, scale, rad_scale=None, exclude_diag=False, band=BAND):
    """bool [Na, Nb]: pairs whose decision d2 <= rad2_b[j] is not held exactly.  rad_scale None (the radii are exact inputs of the
    scan): |d2 - rad2| <= band * (|a|^2 + |b|^2).  rad_scale [Nb] (the radii are computed distances themselves, of pairs with that
    |.|^2 + |.|^2): each side is within band / 2 of its own scale by the accuracy bound, so |d2 - rad2| <= band / 2 * (scale + rad_scale)"""
    thr = band * scale if rad_scale is None else 0.5 * band * (scale + np.asarray(rad_scale, np.float64)[None, :])
    m = np.abs(np.asarray(d2, np.float64) - np.asarray(rad2_b, np.float64)[None, :]) <= thr
    if exclude_diag:
        n = min(m.shape)
        m[np.arange(n), np.arange(n)] = False
    return m


def moments_ref(x, shift):
    """fp64 (sum [D], gram [D, D] full, n) of fl32(x - shift)"""
    y = (np.asarray(x, np.float32) - np.asarray(shift, np.float32)[None, :]).astype(np.float32).astype(np.float64)
    return y.sum(axis=0), y.T @ y, y.shape[0]


def mean_cov(x):
    x = np.asarray(x, np.float64)
    return {"n": x.shape[0], "mean": x.mean(axis=0), "cov": np.cov(x, rowvar=False, ddof=1).reshape(x.shape[1], x.shape[1])}


def frechet_eigh(mr, mf):
    """the symmetric form: tr (S_r^1/2 S_f S_r^1/2)^1/2 through two eigh decompositions; eigenvalues of the product below D eps of
    the largest count as the zeros they are, and the value is clamped at 0"""
    w, v = np.linalg.eigh(mr["cov"])
    root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = root @ mf["cov"] @ root
    ev = np.linalg.eigvalsh((m + m.T) * 0.5)
    ev[ev <= ev.size * 2.0 ** -52 * max(ev.max(), 0.0)] = 0.0          # the exact zeros of a rank-deficient product, +-rounding
    d = mr["mean"] - mf["mean"]
    return max(float(d @ d + np.trace(mr["cov"]) + np.trace(mf["cov"]) - 2.0 * np.sqrt(ev).sum()), 0.0)


def fd_sensitivity(xr, xf):
    """how far the fp64 Frechet term itself moves when only the summation order of its moments changes (rows reversed; sums and Gram
    matrix instead of np.cov): on rank-deficient covariances the square roots of rounding-level eigenvalues carry ~1e-8 of the value.
    -> the largest such difference: the unit of the tolerance for any other exact-sum implementation"""
    base = frechet_eigh(mean_cov(xr), mean_cov(xf))

    def from_sums(x):
        s, g, n = moments_ref(x, np.zeros(x.shape[1], np.float32))
        mean = s / n
        return {"n": n, "mean": mean, "cov": (g - n * np.outer(mean, mean)) / (n - 1)}

    variants = [frechet_eigh(mean_cov(xr[::-1]), mean_cov(xf[::-1])), frechet_eigh(from_sums(xr), from_sums(xf)),
                frechet_eigh(from_sums(xr[::-1]), from_sums(xf[::-1]))]
    return max(abs(v - base) for v in variants)


def set_metrics_ref(real, fake, k):
    """the five numbers in fp64 on the centred fp32 features, plus what the in-band pairs allow each to move by:
    -> (metrics dict, slack dict, in-band row fractions dict)"""
    xr, xf = centre(real, fake)
    nr, nf = xr.shape[0], xf.shape[0]
    d_rr, d_ff, d_fr = d2_fp64(xr, xr), d2_fp64(xf, xf), d2_fp64(xf, xr)
    d_rf = d_fr.T
    rad_r = pair_scan_ref(xr, xr, k, exclude_diag=True, d2=d_rr)[0][:, k - 1]
    rad_f = pair_scan_ref(xf, xf, k, exclude_diag=True, d2=d_ff)[0][:, k - 1]
    c_fr = (d_fr <= rad_r[None, :]).sum(axis=1)
    c_rf = (d_rf <= rad_f[None, :]).sum(axis=1)
    near = d_rf.min(axis=1)
    m = {"precision": float(np.mean(c_fr > 0)), "recall": float(np.mean(c_rf > 0)), "density": float(c_fr.sum() / (k * nf)),
         "coverage": float(np.mean(near <= rad_r)), "fd": frechet_eigh(mean_cov(xr), mean_cov(xf)), "k": k, "n_real": nr, "n_fake": nf,
         "dim": xr.shape[1]}
    # a radius is itself a computed distance, of the pair (j, its k-th neighbour): in_band's rad_scale
    sq_r, sq_f = (xr.astype(np.float64) ** 2).sum(axis=1), (xf.astype(np.float64) ** 2).sum(axis=1)
    rs_r = sq_r + sq_r[pair_scan_ref(xr, xr, k, exclude_diag=True, d2=d_rr)[1][:, k - 1]]
    rs_f = sq_f + sq_f[pair_scan_ref(xf, xf, k, exclude_diag=True, d2=d_ff)[1][:, k - 1]]
    s_fr = norm_scale(xf, xr)
    s_rf = s_fr.T
    band_fr = in_band(d_fr, rad_r, s_fr, rad_scale=rs_r)
    band_rf = in_band(d_rf, rad_f, s_rf, rad_scale=rs_f)
    # coverage compares a real's nearest fake with the real's own radius: the scale of any fake that could be the computed nearest
    cand = d_rf <= near[:, None] + BAND * s_rf
    band_cov = np.abs(near - rad_r) <= 0.5 * BAND * (np.where(cand, s_rf, 0.0).max(axis=1) + rs_r)
    rows_fr, rows_rf = band_fr.any(axis=1), band_rf.any(axis=1)
    slack = {"precision": float(rows_fr.sum() / nf), "recall": float(rows_rf.sum() / nr), "density": float(band_fr.sum() / (k * nf)),
             "coverage": float(band_cov.sum() / nr)}
    return m, slack, {"fr": float(rows_fr.mean()), "rf": float(rows_rf.mean())}
