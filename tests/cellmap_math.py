"""Numpy restatements of the per-cell maps (docs/design/30-cell-maps.md), shared by tests/test_cellmap_cpu.py and
tests/test_gpu_cellmap.py.  TEST INFRASTRUCTURE -- never imported by the product package.

  * recon_cells_ref      fp64: dvq_recon_cells by its definition in include/dvq_hip.h, on the fp64 restatement of tests/test_eval_cpu.py
  * recon_cells_f32      the same formula in numpy float32 with the kernel's staging (v01 - 0.5 rounded to fp32, fp32 moments, horizontal
                         then vertical 11-tap pass): what fp32 arithmetic alone costs a cell's SSIM, computable without a GPU
  * forward_back         DualGrainSeperatePermuter.forward_back restated sequentially; it also reports the cell every sequence entry is
                         written into, which is the attribution rule of the likelihood maps
  * nll_cells_ref        dvq_nll_cell_sums through that attribution, fp64
"""
import numpy as np

from test_eval_cpu import gaussian11, ssim_terms, to01

STREAMS = ("content_coarse", "content_fine", "position_coarse", "position_fine")

# (image H, W, cell grid hg, wg): the smallest shapes at which attribution can go wrong, and the product shape
RECON_SHAPES = [(16, 16, 1, 1), (32, 32, 2, 2), (48, 80, 3, 5), (64, 64, 2, 2), (32, 32, 4, 4), (256, 256, 16, 16)]
RECON_KINDS = ("random", "smooth", "saturated")


def image_pair(kind, b, h, w, seed):
    """x, y fp32 [b, 3, h, w]: random = independent uniform images; smooth = a low-frequency image and a slightly blurred, shifted copy
    (flat cells: the hard case for a cell's SSIM); saturated = values beyond [-1, 1] on both sides (the clamp is exercised)"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        x = rng.uniform(-1, 1, (b, 3, h, w))
        y = np.clip(x + rng.normal(0, 0.2, x.shape), -1, 1)
    elif kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        ph = rng.uniform(0, 6.28, (b, 3, 1, 1))
        x = 0.6 * np.sin(xx / 23.0 + ph) * np.cos(yy / 17.0 - ph) + 0.1
        y = x + 0.01 * np.sin(xx / 5.0 + yy / 7.0) + 0.004
    elif kind == "saturated":
        x = rng.uniform(-1.6, 1.6, (b, 3, h, w))
        y = np.where(rng.uniform(size=x.shape) < 0.5, x, rng.uniform(-1.6, 1.6, x.shape))
    else:
        raise ValueError(kind)
    return x.astype(np.float32), y.astype(np.float32)


def window_counts(h, w, hg, wg):
    """[hg, wg] valid windows whose top-left pixel lies in each cell, by counting"""
    ch, cw = h // hg, w // wg
    n = np.zeros((hg, wg), dtype=np.int64)
    for r in range(max(h - 10, 0)):
        for c in range(max(w - 10, 0)):
            n[r // ch, c // cw] += 1
    return n


def _cell_sums(a, hg, wg, ch, cw):
    """a [B, C, R, S] with R <= hg * ch, S <= wg * cw (a map that may stop short of the image) -> [B, hg, wg] sums over channels and cells"""
    b = a.shape[0]
    full = np.zeros((b, a.shape[1], hg * ch, wg * cw), dtype=np.float64)
    full[:, :, :a.shape[2], :a.shape[3]] = a
    return full.reshape(b, a.shape[1], hg, ch, wg, cw).sum(axis=(1, 3, 5))


def recon_cells_ref(x, y, hg, wg, quantize_u8=False):
    """fp64 [B, hg, wg, 3] by the definition of dvq_recon_cells"""
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    b, _, h, w = x64.shape
    ch, cw = h // hg, w // wg
    x01, y01 = to01(x64, quantize_u8), to01(y64, quantize_u8)
    out = np.zeros((b, hg, wg, 3), dtype=np.float64)
    out[..., 0] = _cell_sums((x01 - y01) ** 2, hg, wg, ch, cw)
    out[..., 1] = _cell_sums(np.abs(x64 - y64), hg, wg, ch, cw)
    if h >= 11 and w >= 11:
        lum, cs = ssim_terms(x01, y01)
        out[..., 2] = _cell_sums(lum * cs, hg, wg, ch, cw)
    return out


def ssim_map_f32(x, y, quantize_u8=False):
    """the SSIM map [B, 3, H - 10, W - 10] in float32 with the kernel's staging: v01 - 0.5 rounded to fp32, every product and sum in fp32,
    taps added in index order, horizontal pass first"""
    f = np.float32
    sx = (to01(np.asarray(x, dtype=np.float64), quantize_u8) - 0.5).astype(f)
    sy = (to01(np.asarray(y, dtype=np.float64), quantize_u8) - 0.5).astype(f)
    g = gaussian11().astype(f)
    h, w = sx.shape[-2:]

    def filt(a):
        r = np.zeros(a.shape[:-1] + (w - 10,), dtype=f)
        for k in range(11):
            r = (r + g[k] * a[..., :, k:w - 10 + k]).astype(f)
        o = np.zeros(a.shape[:-2] + (h - 10, w - 10), dtype=f)
        for k in range(11):
            o = (o + g[k] * r[..., k:h - 10 + k, :]).astype(f)
        return o
    mx, my = filt(sx), filt(sy)
    mxx, myy, mxy = filt((sx * sx).astype(f)), filt((sy * sy).astype(f)), filt((sx * sy).astype(f))
    vx, vy, cxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    ux, uy = mx + f(0.5), my + f(0.5)
    c1, c2 = f(0.01) * f(0.01), f(0.03) * f(0.03)
    num = (f(2) * ux * uy + c1) * (f(2) * cxy + c2)
    den = (ux * ux + uy * uy + c1) * (vx + vy + c2)
    out = num / den
    assert out.dtype == f
    return out


def recon_cells_f32(x, y, hg, wg, quantize_u8=False):
    """[B, hg, wg] per-cell SSIM sums of ssim_map_f32 (the sums themselves in fp64, like the kernel's)"""
    h, w = x.shape[-2:]
    if h < 11 or w < 11:
        return np.zeros((x.shape[0], hg, wg))
    return _cell_sums(ssim_map_f32(x, y, quantize_u8).astype(np.float64), hg, wg, h // hg, w // wg)


def cell_mean_deviation(a_sums, b_sums, h, w, hg, wg):
    """largest |a - b| of the per-cell MEAN SSIM (sum / (3 * windows)) over the cells that have a window"""
    n = 3.0 * window_counts(h, w, hg, wg)
    m = n > 0
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a_sums - b_sums)[:, m] / n[m]))


def ssim_f32_yardstick(shapes=None, kinds=RECON_KINDS, quantize=(False, True), b=2):
    """the bound's base: the largest per-cell-mean deviation of the float32 restatement from the fp64 one over the test's cases"""
    worst = 0.0
    for (h, w, hg, wg) in (shapes or RECON_SHAPES):
        for kind in kinds:
            x, y = image_pair(kind, b, h, w, seed=h * 131 + w + hg)
            for q in quantize:
                d = cell_mean_deviation(recon_cells_f32(x, y, hg, wg, q), recon_cells_ref(x, y, hg, wg, q)[..., 2], h, w, hg, wg)
                worst = max(worst, d)
    return worst


# ---- likelihood maps -----------------------------------------------------------------------------------------------------------------
def forward_back(coarse_content, fine_content, coarse_position, fine_position, hw1, hw2, cpos_eos, fpos_eos):
    """DualGrainSeperatePermuter.forward_back, sequentially: coarse codes are gathered until the coarse <eos> and broadcast over their
    cells only if it is present, then fine codes are written until the fine <eos>.  A position that is no grid position (start tokens,
    pad) writes nothing.  -> (code map [B, fhw, fhw], coarse_cell [B, Lc], fine_cell [B, Lf]): the cell (row-major on the hw1 grid) an
    entry is written into, -1 for an entry that writes nothing"""
    cc, fc = np.asarray(coarse_content, dtype=np.int64), np.asarray(fine_content, dtype=np.int64)
    cp, fp = np.asarray(coarse_position, dtype=np.int64), np.asarray(fine_position, dtype=np.int64)
    b = cc.shape[0]
    fhw = hw1 * hw2
    out = np.zeros((b, fhw, fhw), dtype=np.int64)
    ccell = np.full(cc.shape, -1, dtype=np.int64)
    fcell = np.full(fc.shape, -1, dtype=np.int64)
    for i in range(b):
        coarse = np.zeros((hw1, hw1), dtype=np.int64)
        for k in range(cc.shape[1]):
            p = int(cp[i, k])
            if p == cpos_eos:
                out[i] = coarse.repeat(hw2, axis=0).repeat(hw2, axis=1)
                break
            if 0 <= p < hw1 * hw1:
                coarse[p // hw1, p % hw1] = cc[i, k]
                ccell[i, k] = p
        for k in range(fc.shape[1]):
            e = int(fp[i, k])
            if e == fpos_eos:
                break
            if 0 <= e < fhw * fhw:
                r, c = e // fhw, e % fhw
                out[i, r, c] = fc[i, k]
                fcell[i, k] = (r // hw2) * hw1 + c // hw2
    return out, ccell, fcell


def code_cells(hw1, hw2, cpos_eos, fpos_eos):
    """(cell of every coarse position code, cell of every fine position code), read off forward_back on the sequences of all codes"""
    nc, nf = hw1 * hw1, (hw1 * hw2) ** 2
    cp = np.concatenate([np.arange(nc), [cpos_eos]])[None]
    fp = np.concatenate([np.arange(nf), [fpos_eos]])[None]
    _, ccell, fcell = forward_back(np.zeros_like(cp), np.zeros_like(fp), cp, fp, hw1, hw2, cpos_eos, fpos_eos)
    return ccell[0, :nc], fcell[0, :nf]


def _add(cells, outside, i, s, cell, nll, rk):
    tgt = cells[i, s, cell] if cell >= 0 else outside[i, s]
    tgt += np.array([nll, 1.0, float(rk == 0), float(rk < 5)])


def nll_cells_ref(rows, inputs, hw1, hw2, cpos_eos, fpos_eos):
    """rows: {"content" | "coarse_position" | "fine_position": (nll [B, Tp], rank [B, Tp], target [B, Tp])}, the per-row outputs of
    dvq_token_nll for the three losses with the target vectors they were taken against; inputs: the transformer's input streams
    (coarse_content, fine_content, coarse_position, fine_position, start tokens included).  -> (cells fp64 [B, 4, hw1^2, 4], outside
    fp64 [B, 4, 4]).  Content row r targets entry r + 1 of cat(coarse, fine) and goes where forward_back writes that entry; a position
    row goes to the cell of its target code; rank < 0 (ignored) adds nothing."""
    cc, fc = np.asarray(inputs["coarse_content"]), np.asarray(inputs["fine_content"])
    cp, fp = np.asarray(inputs["coarse_position"]), np.asarray(inputs["fine_position"])
    b, lc = cc.shape
    t = lc + fc.shape[1] - 1
    _, ccell, fcell = forward_back(cc, fc, cp, fp, hw1, hw2, cpos_eos, fpos_eos)
    entry_cell = np.concatenate([ccell, fcell], axis=1)
    coarse_of, fine_of = code_cells(hw1, hw2, cpos_eos, fpos_eos)
    cells = np.zeros((b, 4, hw1 * hw1, 4), dtype=np.float64)
    outside = np.zeros((b, 4, 4), dtype=np.float64)
    nll, rank, _ = rows["content"]
    for i in range(b):
        for r in range(nll.shape[1]):
            if rank[i, r] < 0:
                continue
            assert r < t, "a live content row past the sequence"
            _add(cells, outside, i, 0 if r + 1 < lc else 1, entry_cell[i, r + 1], float(nll[i, r]), int(rank[i, r]))
    for name, s, table in (("coarse_position", 2, coarse_of), ("fine_position", 3, fine_of)):
        nll, rank, target = rows[name]
        for i in range(b):
            for r in range(nll.shape[1]):
                if rank[i, r] < 0:
                    continue
                code = int(target[i, r])
                _add(cells, outside, i, s, int(table[code]) if 0 <= code < table.size else -1, float(nll[i, r]), int(rank[i, r]))
    return cells, outside


def grain_token_counts(grain):
    """[B, 4, hw1^2] tokens per stream and cell that follow from a dual grain map [B, hw1, hw1]: a coarse cell holds 1 content and 1
    position token in the coarse streams, a fine cell 4 + 4 in the fine streams"""
    g = np.asarray(grain).reshape(grain.shape[0], -1)
    out = np.zeros((g.shape[0], 4, g.shape[1]), dtype=np.float64)
    out[:, 0] = out[:, 2] = g == 0
    out[:, 1] = out[:, 3] = 4.0 * (g == 1)
    return out
