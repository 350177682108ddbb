"""numpy fp64 restatement of the stage-2 transformer's row and pointwise operations (csrc/transformer.hip and the softmax / transpose
part of csrc/misc.hip; docs/design/25-stage2-kernel-pins.md): what the kernels must compute, written without reference to how they
compute it.  The dropout mask is the one exception: it is an ABI contract (include/dvq_hip.h), so its mirror is integer arithmetic
that has to reproduce the device bit for bit."""
import math

import numpy as np

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def f64(a):
    return np.asarray(a, dtype=np.float64)


def bf16_round(a):
    """fp32 -> nearest bf16 (ties to even) -> fp32, finite values"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps=1e-5):
    """x [rows, C] -> y, mean [rows], rstd [rows] (biased variance)"""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd(x, dy, gamma, eps=1e-5, dres=None, mean=None, rstd=None):
    """-> dx (+ dres), dgamma, dbeta.  mean / rstd: the statistics the forward saved (default: those of x)"""
    x, dy, gamma = f64(x), f64(dy), f64(gamma)
    if mean is None or rstd is None:
        _, mean, rstd = layernorm_fwd(x, gamma, np.zeros_like(gamma), eps)
    mean, rstd = f64(mean)[:, None], f64(rstd)[:, None]
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(axis=1, keepdims=True) - xh * (g * xh).mean(axis=1, keepdims=True))
    if dres is not None:
        dx = dx + f64(dres)
    return dx, (dy * xh).sum(axis=0), dy.sum(axis=0)


# ---- GELU (erf form) ----------------------------------------------------------------------------------------------------------------
def gelu(x):
    x = f64(x)
    return 0.5 * x * _erfc(-x * math.sqrt(0.5))          # 1 + erf(t) = erfc(-t) without the cancellation in the left tail


def gelu_grad(x):
    x = f64(x)
    return 0.5 * _erfc(-x * math.sqrt(0.5)) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---- softmax ------------------------------------------------------------------------------------------------------------------------
def softmax_rows(s, scale):
    z = f64(s) * float(scale)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax_rows_bwd(p, dp, scale):
    """ds = scale p (dp - sum p dp)"""
    p, dp = f64(p), f64(dp)
    return float(scale) * p * (dp - (p * dp).sum(axis=1, keepdims=True))


def causal_valid(rows, length, tq, offset):
    """number of visible columns of every row: min(L, r % Tq + offset + 1)"""
    return np.minimum(length, np.arange(rows, dtype=np.int64) % tq + offset + 1)


def softmax_causal(s, tq, offset, scale):
    """s [rows, L]; row r sees columns <= r % Tq + offset (clipped to L); the others are exactly 0"""
    s = f64(s)
    rows, length = s.shape
    vis = np.arange(length)[None, :] < causal_valid(rows, length, tq, offset)[:, None]
    z = np.where(vis, s * float(scale), -np.inf)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return np.where(vis, e / e.sum(axis=1, keepdims=True), 0.0)


# ---- cross entropy ------------------------------------------------------------------------------------------------------------------
def cross_entropy(logits, v, target, ignore_index, gscale=1.0):
    """logits [rows, ldl], classes = the first v columns.  -> (loss sum, count, dlogits [rows, ldl]) with
    dlogits = gscale (softmax - onehot) in live rows' first v columns and exact zeros elsewhere"""
    logits, target = f64(logits), np.asarray(target, dtype=np.int64)
    z = logits[:, :v]
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    ssum = e.sum(axis=1, keepdims=True)
    live = target != ignore_index
    r = np.nonzero(live)[0]
    lse = (m + np.log(ssum))[:, 0]
    loss = float((lse[r] - z[r, target[r]]).sum())
    d = np.zeros_like(logits)
    p = e / ssum
    p[r, target[r]] -= 1.0
    d[r, :v] = float(gscale) * p[r]
    return loss, int(live.sum()), d


# ---- embeddings ---------------------------------------------------------------------------------------------------------------------
def _idx2d(idx, b):
    idx = np.asarray(idx, dtype=np.int64)
    return np.broadcast_to(idx, (b, idx.shape[-1])) if idx.ndim == 1 else idx      # a shared index row serves every batch entry


def embed_gather(idx, table, out, t0=0, accumulate=False):
    """out [B, Ttot, C]: out[b, t0 + j] (+)= table[idx[b, j]]; the other rows are returned unchanged"""
    out = f64(out).copy()
    idx = _idx2d(idx, out.shape[0])
    ln = idx.shape[1]
    rows = f64(table)[idx]
    out[:, t0:t0 + ln] = out[:, t0:t0 + ln] + rows if accumulate else rows
    return out


def embed_scatter_add(idx, dout, dtable, t0=0, padding_idx=-1):
    """dtable[idx[b, j]] += dout[b, t0 + j]; the padding row receives nothing"""
    dout, dtable = f64(dout), f64(dtable).copy()
    idx = _idx2d(idx, dout.shape[0])
    ln = idx.shape[1]
    keep = idx != padding_idx
    np.add.at(dtable, idx[keep], dout[:, t0:t0 + ln][keep])
    return dtable


def embed_hits(idx, b, v, padding_idx=-1):
    """number of gradient rows every table row receives"""
    idx = _idx2d(idx, b).reshape(-1)
    return np.bincount(idx[idx != padding_idx], minlength=v)


# ---- dropout mask (dvq_common.h: dvq_hash32 / dvq_dropout_seed) --------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def hash32(x):
    x = np.array(x, dtype=np.uint32)
    shape, x = x.shape, x.reshape(-1)                    # (array arithmetic wraps modulo 2^32 without a warning)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x.reshape(shape)


def dropout_seed(seed):
    """64-bit seed -> (rm, ra): the odd multiplier and the offset of the element hash"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & _M32, seed >> 32
    rm = int(hash32(lo ^ 0x9E3779B9)) | 1
    ra = int(hash32((hi + 0x85EBCA6B) & _M32)) ^ int(hash32((lo + 0xC2B2AE35) & _M32))
    return rm, ra


def dropout_threshold(p):
    """(uint32)((double)(float)p * 2^32)"""
    return int(float(np.float32(p)) * 4294967296.0)


def dropout_keep(n, p, seed, start=0):
    """keep[i] for element indices start .. start + n - 1: hash(lo32(i) rm + ra + hi32(i) 0x9E3779B1) >= threshold(p)"""
    rm, ra = dropout_seed(seed)
    i = np.arange(start, start + n, dtype=np.uint64)
    lo, hi = (i & np.uint64(_M32)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32)
    h = hash32(lo * np.uint32(rm) + np.uint32(ra) + hi * np.uint32(0x9E3779B1))
    return h >= np.uint32(dropout_threshold(p))


def dropout_scale(p):
    """the fp32 factor 1 / (1 - p) the kernels multiply kept elements by"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))
