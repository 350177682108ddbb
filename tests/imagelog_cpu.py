"""numpy restatement of the three image-logging kernels (include/dvq_hip.h: dvq_grain_overlay, dvq_grain_lines, dvq_image_grid_u8) and
the seeded inputs of tests/golden/imagelog.npz.  Test infrastructure only: nothing in the package imports it, it is not a fallback.

Every operation is fp32, rounded on its own, divisions are true divisions, float -> byte conversions truncate -- the arithmetic of the
reference's host path (PIL's Image.blend, torch's sub_ / div_ / mul / byte on the CPU, numpy's uint8 casts).  The cell size is H // h
where the reference hard-codes 256 // h.  Shared by tools/gen_golden_imagelog.py (which checks it against the real reference while it
writes the fixture), tests/test_imagelog_cpu.py and tests/test_gpu_imagelog.py.
"""
from __future__ import annotations

import numpy as np

F = np.float32
BLUE, RED = (5, 39, 175), (255, 0, 0)


# ---- arithmetic -------------------------------------------------------------------------------------------------------------------------
def blend_u8(a, b, alpha):
    """PIL's Image.blend(a, b, alpha) per byte: (uint8)(float(a) + float32(alpha) * float(int(b) - int(a))), fp32, truncating"""
    a = np.asarray(a, dtype=np.uint8)
    b = np.asarray(b, dtype=np.uint8)
    diff = (b.astype(np.int32) - a.astype(np.int32)).astype(F)
    step = F(alpha) * diff
    return (a.astype(F) + step).astype(np.int32).astype(np.uint8)


def range_of(v):
    """(lo, d) of image_normalize / make_grid: d = float32(max(double(hi) - double(lo), 1e-5))"""
    lo, hi = F(v.min()), F(v.max())
    return lo, F(max(float(hi) - float(lo), 1e-5))


def unit_bytes(v, lo, d):
    """(uint8)(((v - lo) / d) * 255)"""
    g = (v.astype(F) - lo) / d
    return (g * F(255)).astype(np.int32).astype(np.uint8)


def _cells(m, H, W):
    h, w = m.shape[-2:]
    assert H % h == 0 and W % w == 0 and H // h == W // w, "the map must tile the image in square cells"
    size = H // h
    return size, np.repeat(np.repeat(m, size, axis=-2), size, axis=-1)


def overlay(x, grain=None, score=None, levels=2, low=BLUE, high=RED, scaler=0.9):
    """x fp32 [B,3,H,W]; grain int64 [B,h,w] (levels 2 / 3) or score fp32 [B,h,w] -> fp32 [B,3,H,W] = k / 255"""
    x = np.asarray(x, dtype=F)
    B, _, H, W = x.shape
    m = grain if grain is not None else score
    _, up = _cells(np.asarray(m), H, W)                                   # [B,H,W]
    out = np.empty_like(x)
    for b in range(B):
        lo, d = range_of(x[b])
        p = unit_bytes(x[b], lo, d)                                         # [3,H,W]
        for c in range(3):
            if grain is not None and levels == 2:
                s = up[b].astype(np.int64)
                col = (np.int64(high[c]) * s + np.int64(low[c]) * (1 - s)).astype(np.uint8)      # wraps like np.uint8(int64 array)
            else:
                s = up[b].astype(F) / F(2) if grain is not None else up[b].astype(F)
                hs = F(high[c]) * s
                lt = F(low[c]) * (F(1) - s)
                col = (hs + lt).astype(np.int32).astype(np.uint8)
            k = blend_u8(p[c], col, scaler)
            out[b, c] = k.astype(F) / F(255)
    return out


def line_mask(grain, H, W):
    """bool [B,H,W]: the pixels draw_dual_grain_256res / draw_triple_grain_256res set to -1"""
    grain = np.asarray(grain)
    size, g = _cells(grain, H, W)
    ly = (np.arange(H) % size)[None, :, None]
    lx = (np.arange(W) % size)[None, None, :]

    def on(l):
        hit = l == 0
        hit = hit | ((g >= 1) & (l == size // 2))
        hit = hit | ((g == 2) & ((l == size // 4) | (l == size - size // 4)))
        return hit
    return on(ly) | on(lx)


def lines(x, grain, levels=2):
    x = np.array(x, dtype=F, copy=True)
    B, _, H, W = x.shape
    mask = line_mask(grain, H, W)
    for c in range(3):
        x[:, c][mask] = F(-1)
    return x


def grid_shape(N, H, W, nrow=4, padding=2):
    if N == 1:
        return H, W
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    return (H + padding) * ymaps + padding, (W + padding) * xmaps + padding


def grid_u8(x, nrow=4, padding=2, clamp=True):
    """x fp32 [N,C,H,W], C in {1,3} -> uint8 [GH,GW,3]: clamp, make_grid(nrow, padding, normalize=True), (uint8)(g * 255)"""
    x = np.asarray(x, dtype=F)
    N, C, H, W = x.shape
    assert C in (1, 3)
    if clamp:
        x = np.clip(x, F(-1), F(1))
    if C == 1:
        x = np.concatenate([x, x, x], axis=1)
    lo, d = range_of(x)
    by = unit_bytes(x, lo, d)                                               # [N,3,H,W]
    if N == 1:
        return np.ascontiguousarray(by[0].transpose(1, 2, 0))
    GH, GW = grid_shape(N, H, W, nrow, padding)
    xmaps = min(nrow, N)
    out = np.zeros((GH, GW, 3), dtype=np.uint8)
    for k in range(N):
        y0 = (k // xmaps) * (H + padding) + padding
        x0 = (k % xmaps) * (W + padding) + padding
        out[y0:y0 + H, x0:x0 + W] = by[k].transpose(1, 2, 0)
    return out


# ---- seeded inputs of the fixture (integers from PCG64, then exact or singly rounded fp32 steps: the same bits everywhere) ---------------
FIXTURE_SEED = 1807
FIXTURE_BATCH = 2


def fixture_images(B=FIXTURE_BATCH, H=256, W=256, seed=FIXTURE_SEED):
    """fp32 [B,3,H,W] in [-1, 1]: 16-pixel blocks of seeded bytes under a diagonal ramp"""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, size=(B, 3, -(-H // 16), -(-W // 16)), dtype=np.int64)
    up = np.repeat(np.repeat(blocks, 16, axis=2), 16, axis=3)[:, :, :H, :W]
    y = np.arange(H, dtype=np.int64)[None, None, :, None]
    x = np.arange(W, dtype=np.int64)[None, None, None, :]
    c = np.arange(3, dtype=np.int64)[None, :, None, None]
    v = (up + 3 * y + 5 * x + 11 * c) % 256
    return (v.astype(F) / F(127.5) - F(1)).astype(F)


def fixture_grain(B, h, w, levels, seed=FIXTURE_SEED):
    return np.random.default_rng(seed + 10 * levels + h).integers(0, levels, size=(B, h, w), dtype=np.int64)


def fixture_score(B, h, w, seed=FIXTURE_SEED):
    """fp32 [B,h,w] in [0,1] with exact 0, 1 and 0.5 among the entries (what a min/max-normalised entropy map holds)"""
    s = np.random.default_rng(seed + 77).integers(0, 1001, size=(B, h, w), dtype=np.int64).astype(F) / F(1000)
    s[:, 0, 0], s[:, 0, 1], s[:, 0, 2] = F(0), F(1), F(0.5)
    return s.astype(F)
