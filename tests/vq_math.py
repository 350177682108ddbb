"""numpy float64 restatement of the quantiser's training side and of the grain merges, each operation from its definition
(reference: quantize2_mask.py:57-132,157-191, EncoderDual.py:140-150, EncoderTriple.py:150-176, RouterDual.py:35-42).  Imports nothing
from the package.  Inputs are taken as given (round them to the tensor type first) and promoted to float64; the two functions that
say so work in numpy float32 instead: they restate the value a kernel STORES, bit for bit.
docs/design/31-quantiser-kernel-pins.md says which test holds which kernel to which of these."""
import numpy as np


def f64(a):
    return np.asarray(a, dtype=np.float64)


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32.  Finite values and infinities; NaN stays NaN"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    out = r.view(np.float32).copy()
    nan = np.isnan(a)
    out[nan] = a[nan]
    return out.reshape(a.shape)


# ---- gather, straight-through output, commitment loss, backward ------------------------------------------------------------------------
def gather(e, idx):
    """e [K, D], idx [...] -> e[idx] [..., D] (dtype of e)"""
    return np.asarray(e)[np.asarray(idx)]


def straight_through(x, e, idx):
    """x + (e[idx] - x) in float64"""
    x = f64(x)
    return x + (f64(gather(e, idx)) - x)


def straight_through_f32(x, e, idx):
    """fl(x + fl(e[idx] - x)) in float32 arithmetic: the value the gather kernel forms before its store"""
    x = np.asarray(x, dtype=np.float32)
    df = (np.asarray(gather(e, idx), dtype=np.float32) - x).astype(np.float32)
    return (x + df).astype(np.float32)


def straight_through_bf16(x, e, idx):
    """the bf16 store of straight_through_f32 (one round-to-nearest-even), as float32"""
    return bf16_round(straight_through_f32(x, e, idx))


def row_sqerr(x, e, idx):
    """r_n = sum_d (e[idx_n] - x_n)^2"""
    d = f64(gather(e, idx)) - f64(x)
    return (d * d).sum(axis=-1)


def loss_sum(x, e, idx, mask=None):
    """sum_n mask_n sum_d (e - x)^2"""
    r = row_sqerr(x, e, idx)
    return float(r.sum() if mask is None else (f64(mask) * r).sum())


def vq_loss(x, e, idx, mask=None, beta=0.25):
    """(1 + beta) / numel * loss_sum: VectorQuantize2's scalar (commitment beta * mse + the codebook term mse)"""
    return (1.0 + beta) * loss_sum(x, e, idx, mask) / float(np.asarray(x).size)


def backward(g, x, e, idx, mask, coef):
    """g + coef mask (x - e[idx])"""
    m = 1.0 if mask is None else f64(mask)[..., None]
    return f64(g) + float(coef) * m * (f64(x) - f64(gather(e, idx)))


# ---- EMA ---------------------------------------------------------------------------------------------------------------------------------
def code_sums(x, idx, k):
    """-> (sum of the rows of every code [K, D], number of rows of every code [K])"""
    x = f64(x)
    idx = np.asarray(idx).reshape(-1)
    sums = np.zeros((k, x.shape[1]))
    np.add.at(sums, idx, x)
    return sums, np.bincount(idx, minlength=k).astype(np.float64)


def ema_update(n0, s0, cnt, sums, decay, restart_rows=None):
    """n' = n decay + cnt (1 - decay), s' = s decay + sum (1 - decay); with restart rows a code whose n' is not >= 1 is dead:
    n' = 1, s' = its restart row.  -> (n', s', dead [K] bool; all False without restart rows)"""
    n1 = f64(n0) * decay + f64(cnt) * (1.0 - decay)
    s1 = f64(s0) * decay + f64(sums) * (1.0 - decay)
    dead = np.zeros(n1.shape, dtype=bool)
    if restart_rows is not None:
        dead = ~(n1 >= 1.0)
        n1 = np.where(dead, 1.0, n1)
        s1 = np.where(dead[:, None], f64(restart_rows), s1)
    return n1, s1, dead


def ema_normalize(n1, s1, eps):
    """w_k = s'_k / (n_tot (n'_k + eps) / (n_tot + K eps)), n_tot = sum_k n'_k"""
    n1, s1 = f64(n1), f64(s1)
    tot = n1.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = tot * (n1 + eps) / (tot + n1.shape[0] * eps)
        return s1 / norm[:, None]


# ---- distances ---------------------------------------------------------------------------------------------------------------------------
def distances(x, e):
    """[N, K] squared distances |x_n - e_k|^2"""
    x, e = f64(x), f64(e)
    return ((x[:, None, :] - e[None, :, :]) ** 2).sum(axis=-1)


# ---- merges --------------------------------------------------------------------------------------------------------------------------------
def _up(a, r):
    return np.repeat(np.repeat(a, r, axis=1), r, axis=2)


def dual_merge(h_fine, h_coarse, grain):
    """h_fine [B, 2h, 2w, C], h_coarse [B, h, w, C], grain [B, h, w] (non-zero = fine) -> (merged [B, 2h, 2w, C] in the dtype of
    h_fine: a selection, no arithmetic; mask [B, 2h, 2w]: 1 on fine cells, 0.25 on coarse ones)"""
    fine = _up(np.asarray(grain) != 0, 2)
    out = np.where(fine[..., None], np.asarray(h_fine), _up(np.asarray(h_coarse), 2))
    return out, np.where(fine, 1.0, 0.25)


def dual_merge_bwd(g, grain):
    """-> (g_fine = g on fine cells, 0 elsewhere; g_coarse [B, h, w, C] = the sum of the 2 x 2 gradients of a coarse cell, 0 on fine)"""
    g = f64(g)
    b, h2, w2, c = g.shape
    fine = np.asarray(grain) != 0
    gf = np.where(_up(fine, 2)[..., None], g, 0.0)
    blocks = g.reshape(b, h2 // 2, 2, w2 // 2, 2, c).sum(axis=(2, 4))
    return gf, np.where(fine[..., None], 0.0, blocks)


def dual_merge_bwd_coarse_f32(g, grain):
    """g_coarse as the kernel adds it: from zero, (dy, dx) = (0, 0), (0, 1), (1, 0), (1, 1), in float32"""
    g = np.asarray(g, dtype=np.float32)
    acc = np.zeros_like(g[:, 0::2, 0::2])
    for dy in (0, 1):
        for dx in (0, 1):
            acc = (acc + g[:, dy::2, dx::2]).astype(np.float32)
    return np.where((np.asarray(grain) != 0)[..., None], np.float32(0), acc)


def grain_merge(heads, idx, scale=None):
    """heads [coarsest .. finest], level l [N, hc << l, wc << l, C]; idx [N, hc, wc] the level of a coarsest cell; scale [N, hc, wc] or
    None -> (merged [N, hf, wf, C] = the selected level, nearest-upsampled, times scale; mask [N, hf, wf] = 4^-(S - 1 - level))"""
    s = len(heads)
    f = 1 << (s - 1)
    lvl = _up(np.asarray(idx), f)
    out = np.zeros(heads[-1].shape)
    for l in range(s):
        out = np.where((lvl == l)[..., None], _up(f64(heads[l]), 1 << (s - 1 - l)), out)
    if scale is not None:
        out = out * _up(f64(scale), f)[..., None]
    return out, 4.0 ** -(s - 1 - lvl).astype(np.float64)


def _pool_sum(a, r):
    n, h, w, c = a.shape
    return a.reshape(n, h // r, r, w // r, r, c).sum(axis=(2, 4))


def grain_merge_bwd(g, heads, idx, scale=None):
    """-> ([d head_l]: scale x the sum of the gradients of the finest pixels a pixel of the selected level covers, 0 at the other levels;
    dscale [N, hc, wc] = sum over the cell of g x the selected (upsampled) value;
    acc_abs [N, hc, wc] = sum |summed gradient| |selected value|: the magnitude behind dscale)"""
    s = len(heads)
    g = f64(g)
    idx = np.asarray(idx)
    sc = 1.0 if scale is None else f64(scale)
    dheads, dscale, mag = [], np.zeros(idx.shape), np.zeros(idx.shape)
    for l in range(s):
        acc = _pool_sum(g, 1 << (s - 1 - l))                         # per pixel of level l
        sel = _up(idx == l, 1 << l)[..., None]
        scl = sc if scale is None else _up(sc, 1 << l)[..., None]
        dheads.append(np.where(sel, acc * scl, 0.0))
        prod = np.where(sel, acc * f64(heads[l]), 0.0)
        dscale += _pool_sum(prod, 1 << l).sum(axis=-1)
        mag += _pool_sum(np.abs(prod), 1 << l).sum(axis=-1)
    return dheads, dscale, mag


# ---- pools ---------------------------------------------------------------------------------------------------------------------------------
def avgpool(x, k):
    """x [N, h k, w k, C] -> the mean over k x k windows [N, h, w, C]"""
    return _pool_sum(f64(x), k) / float(k * k)


def avgpool_bwd(dy, k):
    """dy [N, h, w, C] -> dx [N, h k, w k, C] = dy of the window / k^2"""
    return _up(f64(dy), k) / float(k * k)
