"""Reconstruction evaluation of a DQ-VAE: PSNR / SSIM / L1 (+ LPIPS when pretrained weights exist), codebook usage, perplexity
and tokens per image (docs/design/13-evaluation.md); likelihood evaluation of a DQ-Transformer: nats per token, perplexity, top-1 /
top-5 accuracy per token stream, bits per image and per pixel (docs/design/15-likelihood.md).

  * ReconstructionMeter      accumulates batches on the device (csrc/metrics.hip: dvq_recon_metrics, dvq_code_histogram); nothing is
                             copied to the host until summary(), which aggregates in fp64
  * aggregate                the host aggregation of per-image values and code counts (pure numpy: testable without a GPU)
  * evaluate_reconstruction  one model.ae_fwd(x, None) per batch in eval mode under no_grad: reconstruction, code map and grain map
                             of entropy-routed and feature-routed dual / triple grain models from one pass; no EMA update

  * LikelihoodMeter          accumulates Dualformer.score blocks ([B, 4, 4] fp64) on the device, one host copy in summary()
  * aggregate_likelihood     host aggregation of the per-image stream sums (pure numpy)
  * evaluate_likelihood      one model.score per batch (teacher forcing, eval mode, no gradient)

  * CellMeter                accumulates per-cell error maps (dvq_recon_cells), patch entropies, grain maps and per-cell likelihood maps
                             (dvq_nll_cell_sums) on the device; summary() makes the one host copy (docs/design/30-cell-maps.md)
  * aggregate_cells          host aggregation of the maps: by grain, by entropy decile, Spearman rank correlations, consistency with the
                             per-image figures (pure numpy)
  * evaluate_cells           one ae_fwd (+ one score_cells) per batch

  * sample_set_metrics       Frechet distance, improved precision / recall, density / coverage of a fake feature set against a real one:
                             two dvq_feat_moments passes and four dvq_pair_scan scans on the device, the reduction on the host
                             (docs/design/32-sample-set-metrics.md); frechet_distance / moments_from_sums are its host half (pure numpy)
  * evaluate_samples         the same on the frozen DQ-VAE's pooled encoder features (model.pooled_features) of two image streams

`reference_usage` reproduces what the reference's scripts/tools/codebook_usage_dqvae.py:69 prints under the label "usage":
1 - codes_used / K, i.e. the UNUSED fraction of the codebook.
"""
from __future__ import annotations

import numpy as np
import torch

from . import kernels as K
from . import runtime as rt

LPIPS_NOTE = ("lpips not reported: pretrained VGG16 / LPIPS lin weights were not found ($DVQ_VGG16_WEIGHTS, $DVQ_LPIPS_LIN_WEIGHTS); "
              "random-feature LPIPS values are never reported")


def perplexity(counts) -> float | None:
    """exp of the entropy of the frequency distribution `counts` (natural log); None when nothing was counted"""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    n = c.sum()
    if n <= 0:
        return None
    p = c[c > 0] / n
    return float(np.exp(-np.sum(p * np.log(p))))


def tokens_stats(tokens) -> dict:
    """mean / variance / min / max of the per-image token counts (calibrate.sequence_length_stats' keys and types)"""
    t = np.asarray(tokens, dtype=np.int64).reshape(-1)
    if t.size == 0:
        return {"mean": None, "variance": None, "min": None, "max": None}
    return {"mean": float(np.mean(t)), "variance": float(np.var(t)), "min": int(t.min()), "max": int(t.max())}


def aggregate(mse, l1, ssim, counts, tokens, invalid=0, lpips=None) -> dict:
    """host aggregation (fp64).  mse / l1 / ssim: per-image values; counts int [G, K] tokens per (grain, code); tokens: per-image
    token counts; lpips: per-image values or None (-> "lpips": None with a note)."""
    mse = np.asarray(mse, dtype=np.float64).reshape(-1)
    l1 = np.asarray(l1, dtype=np.float64).reshape(-1)
    ssim = np.asarray(ssim, dtype=np.float64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim == 1:
        counts = counts[None]
    n_grains, n_codes = counts.shape
    exact = mse == 0.0
    total = counts.sum(axis=0)
    used = int(np.count_nonzero(total))
    # cells per grain: a cell of grain g spends 4^g tokens (include/dvq_hip.h, dvq_code_histogram)
    cells = np.array([counts[g].sum() / 4.0 ** g for g in range(n_grains)], dtype=np.float64)
    out = {
        "n_images": int(mse.size),
        "l1": float(l1.mean()) if l1.size else None,
        "mse": float(mse.mean()) if mse.size else None,
        "psnr": float(np.mean(10.0 * np.log10(1.0 / mse[~exact]))) if (~exact).any() else None,
        "n_exact": int(exact.sum()),
        "ssim": float(ssim.mean()) if ssim.size else None,
        "lpips": None,
        "codes_used": used,
        "used_fraction": used / n_codes,
        "unused_fraction": 1.0 - used / n_codes,
        "reference_usage": 1.0 - used / n_codes,
        "perplexity": perplexity(total),
        "per_grain": [{"tokens": int(counts[g].sum()), "codes_used": int(np.count_nonzero(counts[g])), "perplexity": perplexity(counts[g])}
                      for g in range(n_grains)],
        "grain_fraction": [float(c / cells.sum()) for c in cells] if cells.sum() > 0 else [None] * n_grains,
        "tokens_per_image": tokens_stats(tokens),
        "invalid": int(invalid),
    }
    if lpips is not None:
        out["lpips"] = float(np.mean(np.asarray(lpips, dtype=np.float64)))
    else:
        out["lpips_note"] = LPIPS_NOTE
    return out


class ReconstructionMeter:
    """Accumulates per-image MSE / L1 / SSIM and the grain-aware code histogram of evaluation batches on the device.

    update(x, rec, codes, grain): x / rec NCHW fp32 [B,3,H,W] in [-1, 1]; codes int64 [B,Hf,Wf] (VectorQuantize2's code map); grain int64
    [B,hg,wg] (the model's grain map, 0 = coarsest) or None for a single-grain code map.  Only kernel launches: the per-image results
    stay on the device until summary()."""

    def __init__(self, n_codes: int, n_grains: int = 1, quantize_u8: bool = True):
        self.n_codes, self.n_grains, self.quantize_u8 = int(n_codes), int(n_grains), bool(quantize_u8)
        self.counts = self.invalid = None
        self._ws = {}
        self._per_image = []          # (mse, l1, ssim, tokens) device tensors per batch
        self._lpips = []

    def update(self, x, rec, codes, grain=None, lpips=None):
        if self.counts is None:
            self.counts = torch.zeros(self.n_grains, self.n_codes, dtype=torch.int64, device=x.device)
            self.invalid = torch.zeros(1, dtype=torch.int64, device=x.device)
        b, _, h, w = x.shape
        ws = self._ws.get((b, h, w))
        if ws is None:
            ws = self._ws[(b, h, w)] = K.recon_metrics_workspace(b, h, w, x.device)
        mse, l1, ssim = K.recon_metrics(x, rec, self.quantize_u8, ws)
        tokens = K.code_histogram(codes, grain, self.n_codes, self.n_grains, self.counts, self.invalid)
        self._per_image.append((mse, l1, ssim, tokens))
        if lpips is not None:
            self._lpips.append(lpips.reshape(-1))

    def summary(self) -> dict:
        """copies the accumulated device values to the host (the only synchronisation of the meter) and aggregates them in fp64"""
        if not self._per_image:
            raise ValueError("ReconstructionMeter.summary(): no batch was added")
        cols = [np.concatenate([t[i].cpu().numpy() for t in self._per_image]) for i in range(4)]
        lp = np.concatenate([t.float().cpu().numpy() for t in self._lpips]) if self._lpips else None
        if lp is not None and lp.size != cols[0].size:
            raise ValueError("lpips values were given for some batches only")
        return aggregate(cols[0], cols[1], cols[2], self.counts.cpu().numpy(), cols[3], int(self.invalid.cpu()[0]), lpips=lp)


def dtype_name() -> str:
    if rt.compute_dtype() == torch.bfloat16:
        return "bf16"
    return "fp32x3" if rt.fp32_split() else "fp32"


def _lpips_module(lpips, device):
    """None -> losses.LPIPS() when its pretrained weights are found; False -> no LPIPS; a module -> used iff pretrained_loaded"""
    if lpips is False:
        return None
    if lpips is None:
        from .losses import LPIPS
        lpips = LPIPS()
    if not getattr(lpips, "pretrained_loaded", False):
        return None
    return lpips.to(device).eval()


def evaluate_reconstruction(model, batches, quantize_u8: bool = True, lpips=None, on_batch=None) -> dict:
    """Reconstruction quality and codebook usage of a DQ-VAE over `batches` (NCHW fp32 [B,3,H,W] tensors in [-1, 1], or dicts holding
    one under model.image_key).  One model.ae_fwd(x, None) per batch, in eval mode under no_grad: the EMA buffers and the codebook
    are not touched.  lpips: None (losses.LPIPS() if its pretrained weights are found), False, or an LPIPS module (used only if
    pretrained_loaded).  on_batch(x, out): optional callback with the batch and ae_fwd's output dict.
    Keys: see aggregate(), plus ema_dead_codes (codes with cluster_size_ema < 1) and dtype."""
    model.eval()
    from .quantize import codebook_of
    weight, n_codes = codebook_of(model.quantize)
    cbk = getattr(model.quantize, "codebook", None)          # the EMA quantiser's embedding (None for a gradient-trained codebook)
    meter = ReconstructionMeter(n_codes, model.N_GRAINS, quantize_u8=quantize_u8)
    lp_mod = _lpips_module(lpips, weight.device)
    with torch.no_grad():
        for batch in batches:
            x = batch[getattr(model, "image_key", "image")] if isinstance(batch, dict) else batch
            x = x.float().contiguous() if x.dtype != torch.float32 or not x.is_contiguous() else x
            out = model.ae_fwd(x, None)
            lv = lp_mod(x, out["rec"]).reshape(-1) if lp_mod is not None else None
            meter.update(x, out["rec"], out["codes"], out["grain"], lpips=lv)
            if on_batch is not None:
                on_batch(x, out)
    s = meter.summary()
    ema = getattr(cbk, "cluster_size_ema", None)
    s["ema_dead_codes"] = int((ema.detach().cpu().numpy() < 1.0).sum()) if ema is not None else None
    s["dtype"] = dtype_name()
    return s


# ---- stage 2: teacher-forced likelihood of a DQ-Transformer (docs/design/15-likelihood.md) ------------------------------------------------
LIKELIHOOD_STREAMS = ("content_coarse", "content_fine", "position_coarse", "position_fine")     # = StackGPT.SCORE_STREAMS
_LN2 = float(np.log(2.0))


def _div(a, b):
    return float(a / b) if b > 0 else None


def step_losses(sums, content_loss_weight=1.0, position_loss_weight=1.0) -> dict:
    """the losses Dualformer._step logs for ONE batch, from that batch's [4, 4] stream sums (rows LIKELIHOOD_STREAMS, columns nll
    sum / tokens / ...): each loss is the mean over the batch's non-ignored targets (F.cross_entropy's reduction), position =
    (coarse + fine) / 2, loss = content_loss_weight * content + position_loss_weight * position.  A loss without a target is None (the
    training step would log NaN), and so is everything built on it."""
    sums = np.asarray(sums, dtype=np.float64)
    content = _div(sums[0, 0] + sums[1, 0], sums[0, 1] + sums[1, 1])
    coarse, fine = _div(sums[2, 0], sums[2, 1]), _div(sums[3, 0], sums[3, 1])
    position = (coarse + fine) / 2 if coarse is not None and fine is not None else None
    loss = content_loss_weight * content + position_loss_weight * position if content is not None and position is not None else None
    return {"content_loss": content, "position_loss": position, "coarse_position_loss": coarse, "fine_position_loss": fine, "loss": loss}


def aggregate_likelihood(per_image, pixels_per_image=None, content_loss_weight=1.0, position_loss_weight=1.0, batch_sizes=None) -> dict:
    """host aggregation (fp64, pure numpy) of per-image stream sums [N, 4, 4]: axis 1 = LIKELIHOOD_STREAMS, axis 2 = (sum of the
    tokens' negative log-likelihoods in nats, tokens, top-1 hits, top-5 hits).

    streams[name]:    nats_per_token = sum / tokens, perplexity = exp(sum / tokens), top1 / top5 = hits / tokens (all None for a stream
                      without tokens), tokens, tokens_per_image {mean, min, max}
    nats_per_image:   all four streams' sums / N; bits_per_image = nats / ln 2; bits_per_pixel = bits_per_image / pixels_per_image
                      (H * W * 3; None when pixels_per_image is not given)
    loss:             step_losses of the WHOLE set taken as one batch
    loss_batch_mean:  with batch_sizes (how the N images were grouped, in order): the unweighted mean over batches of each batch's
                      step_losses -- what an epoch average of the logged validation losses is for equal batch sizes; None for a loss
                      that some batch lacks"""
    a = np.asarray(per_image, dtype=np.float64)
    if a.ndim != 3 or a.shape[1:] != (4, 4):
        raise ValueError(f"per-image likelihood sums must be [N, 4, 4], got {a.shape}")
    n = a.shape[0]
    tot = a.sum(axis=0)
    streams = {}
    for i, name in enumerate(LIKELIHOOD_STREAMS):
        npt = _div(tot[i, 0], tot[i, 1])
        tok = a[:, i, 1]
        with np.errstate(over="ignore"):
            streams[name] = {"nats_per_token": npt, "perplexity": float(np.exp(npt)) if npt is not None else None,
                             "top1": _div(tot[i, 2], tot[i, 1]), "top5": _div(tot[i, 3], tot[i, 1]), "tokens": int(tot[i, 1]),
                             "tokens_per_image": {"mean": float(tok.mean()) if n else None, "min": int(tok.min()) if n else None,
                                                  "max": int(tok.max()) if n else None}}
    nats = _div(tot[:, 0].sum(), n)
    bits = nats / _LN2 if nats is not None else None
    all_tok = a[:, :, 1].sum(axis=1)
    out = {"n_images": int(n), "streams": streams, "nats_per_image": nats, "bits_per_image": bits,
           "bits_per_pixel": bits / float(pixels_per_image) if bits is not None and pixels_per_image else None,
           "pixels_per_image": int(pixels_per_image) if pixels_per_image else None,
           "tokens_per_image": {"mean": float(all_tok.mean()) if n else None, "min": int(all_tok.min()) if n else None,
                                "max": int(all_tok.max()) if n else None},
           "content_loss_weight": float(content_loss_weight), "position_loss_weight": float(position_loss_weight),
           "loss": step_losses(tot, content_loss_weight, position_loss_weight), "loss_batch_mean": None}
    if batch_sizes is not None:
        sizes = [int(b) for b in batch_sizes]
        if sum(sizes) != n or any(b <= 0 for b in sizes):
            raise ValueError(f"batch_sizes {sizes} do not partition {n} images")
        per_batch, i0 = [], 0
        for b in sizes:
            per_batch.append(step_losses(a[i0:i0 + b].sum(axis=0), content_loss_weight, position_loss_weight))
            i0 += b
        out["loss_batch_mean"] = {k: (float(np.mean([p[k] for p in per_batch])) if all(p[k] is not None for p in per_batch) else None)
                                  for k in per_batch[0]} if per_batch else None
    return out


class LikelihoodMeter:
    """Accumulates the [B, 4, 4] blocks of Dualformer.score on the device; summary() makes the one host copy and aggregates in fp64."""

    def __init__(self, content_loss_weight=1.0, position_loss_weight=1.0):
        self.content_loss_weight, self.position_loss_weight = float(content_loss_weight), float(position_loss_weight)
        self._blocks = []
        self.pixels_per_image = None

    def update(self, block, pixels_per_image=None):
        if block.dim() != 3 or tuple(block.shape[1:]) != (4, 4):
            raise ValueError(f"LikelihoodMeter.update: expected [B, 4, 4], got {tuple(block.shape)}")
        self._blocks.append(block)
        if pixels_per_image is not None:
            if self.pixels_per_image not in (None, int(pixels_per_image)):
                raise ValueError("images of different sizes in one likelihood evaluation")
            self.pixels_per_image = int(pixels_per_image)

    def per_image(self):
        """[N, 4, 4] fp64 on the host (one copy)"""
        if not self._blocks:
            raise ValueError("LikelihoodMeter: no batch was added")
        return torch.cat(self._blocks, dim=0).cpu().numpy().astype(np.float64)

    def summary(self, per_image: bool = False) -> dict:
        a = self.per_image()
        out = aggregate_likelihood(a, self.pixels_per_image, self.content_loss_weight, self.position_loss_weight,
                                   batch_sizes=[int(b.shape[0]) for b in self._blocks])
        if per_image:
            out["per_image"] = a
        return out


def token_pixels_per_image(model) -> int:
    """H * W * 3 of the images behind a token batch: the fine grid times the first stage's downsampling, i.e. the resolution its encoder
    was built for"""
    side = int(model.first_stage_model.encoder.resolution)
    return side * side * 3


def evaluate_likelihood(model, batches, per_image: bool = False) -> dict:
    """Teacher-forced likelihood of images under a Dualformer / ClassDualformer: one model.score per batch (frozen DQ-VAE -> codes ->
    permuter -> StackGPT in eval mode, no dropout, no gradient), blocks kept on the device, one host copy at the end.  batches: dicts
    for model.get_xc ({"image": ..., "class_label": ...}), bare image tensors for an unconditional model, or token batches
    ({"tokens": ...} of tokens.TokenBatchLoader: model.score_tokens, no first stage).  Keys: see
    aggregate_likelihood(), plus dtype; per_image=True adds "per_image", the [N, 4, 4] fp64 array."""
    meter = LikelihoodMeter(model.content_loss_weight, model.position_loss_weight)
    with torch.no_grad():
        for batch in batches:
            if isinstance(batch, dict) and "tokens" in batch:
                meter.update(model.score_tokens(*model.get_tc(batch)), pixels_per_image=token_pixels_per_image(model))
                continue
            if isinstance(batch, dict):
                x, c = model.get_xc(batch)
            elif model.cond_stage_key == model.first_stage_key:
                x = c = model.get_input({model.first_stage_key: batch}, model.first_stage_key)
            else:
                raise ValueError(f"a conditional model needs dict batches with '{model.cond_stage_key}'")
            meter.update(model.score(x, c), pixels_per_image=int(x.shape[-2]) * int(x.shape[-1]) * 3)
    s = meter.summary(per_image=per_image)
    s["dtype"] = dtype_name()
    return s


# ---- per-cell maps: where an image's error and its bits fall (docs/design/30-cell-maps.md) ------------------------------------------------
def average_ranks(v):
    """1-based ranks of a 1-d array, ties sharing the average of the ranks they span (fp64)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    order = np.argsort(v, kind="stable")
    sv = v[order]
    ranks = np.empty(v.size, dtype=np.float64)
    start = np.flatnonzero(np.concatenate([[True], sv[1:] != sv[:-1]])) if v.size else np.zeros(0, dtype=np.int64)
    end = np.concatenate([start[1:], [v.size]]) if v.size else start
    for a, b in zip(start, end):
        ranks[order[a:b]] = 0.5 * (a + 1 + b)
    return ranks


def spearman(a, b):
    """Spearman rank correlation with average ranks for ties: Pearson's r of the rank vectors.  None for fewer than two points or a
    constant vector (the coefficient is undefined)"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    if a.size != b.size:
        raise ValueError(f"spearman: {a.size} and {b.size} values")
    if a.size < 2:
        return None
    ra, rb = average_ranks(a), average_ranks(b)
    da, db = ra - ra.mean(), rb - rb.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return float((da * db).sum() / den) if den > 0 else None


def decile_index(values):
    """-> (index in 0..9 per value, the nine inner edges): edges = the 10 %, ..., 90 % quantiles of the pooled values (linear
    interpolation); a value belongs to the decile whose lower edge it reaches (index = number of edges <= value), so equal values always
    share a decile and a decile can be empty when ties straddle an edge"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    edges = np.quantile(v, np.arange(1, 10) / 10.0) if v.size else np.zeros(9)
    return np.searchsorted(edges, v, side="right"), edges


def cell_window_counts(h, w, hg, wg):
    """int64 [hg, wg]: valid 11 x 11 SSIM windows (top-left (r, c), r <= h - 11, c <= w - 11) whose top-left pixel lies in each cell"""
    ch, cw = h // hg, w // wg
    rows = np.clip(np.minimum((np.arange(hg) + 1) * ch, h - 10) - np.arange(hg) * ch, 0, None)
    cols = np.clip(np.minimum((np.arange(wg) + 1) * cw, w - 10) - np.arange(wg) * cw, 0, None)
    return (rows[:, None] * cols[None, :]).astype(np.int64)


def _rel_gap(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.maximum(np.abs(b), np.finfo(np.float64).tiny)
    return float(np.max(np.where(a == b, 0.0, np.abs(a - b) / den))) if a.size else 0.0


def aggregate_cells(h, w, n_grains, grain, recon=None, entropy=None, bits=None, outside=None, ref_recon=None, ref_score=None) -> dict:
    """host aggregation (fp64, pure numpy) of N images' cell maps over an hg x wg grid of an h x w image.
    grain int [N, hg, wg] (0 = coarsest; a cell of grain g spends 4^g content tokens); recon fp64 [N, hg, wg, 3] = dvq_recon_cells' sums
    or None; entropy [N, hg, wg] or None; bits: dvq_nll_cell_sums' cells fp64 [N, 4, hg * wg, 4] with outside [N, 4, 4], or None;
    ref_recon = (mse, l1, ssim) per image and ref_score [N, 4, 4]: the per-image figures the cells must add up to.
    A cell's "bits" are its four streams' nll sums / ln 2; a cell's "error" is its squared-error sum."""
    grain = np.asarray(grain, dtype=np.int64)
    n, hg, wg = grain.shape
    ncell = hg * wg
    pix = (h // hg) * (w // wg) * 3
    win = cell_window_counts(h, w, hg, wg)
    g_flat = grain.reshape(-1)
    sq = ab = ss = ent = cell_bits = None
    if recon is not None:
        recon = np.asarray(recon, dtype=np.float64).reshape(n, hg, wg, 3)
        sq, ab, ss = recon[..., 0].reshape(-1), recon[..., 1].reshape(-1), recon[..., 2].reshape(-1)
    if entropy is not None:
        ent = np.asarray(entropy, dtype=np.float64).reshape(-1)
    if bits is not None:
        bits = np.asarray(bits, dtype=np.float64).reshape(n, 4, ncell, 4)
        outside = np.asarray(outside, dtype=np.float64).reshape(n, 4, 4)
        cell_bits = (bits[:, :, :, 0].sum(axis=1) / _LN2).reshape(-1)
    win_flat = np.broadcast_to(win, (n, hg, wg)).reshape(-1)
    tokens = 4.0 ** g_flat
    by_grain = []
    for g in range(n_grains):
        m = g_flat == g
        k = int(m.sum())
        row = {"grain": g, "cells": k, "cell_share": _div(k, g_flat.size), "token_share": _div(tokens[m].sum(), tokens.sum()),
               "sq_err_share": None, "bits_share": None, "mse": None, "psnr": None, "ssim": None, "bits_per_token": None}
        if sq is not None:
            row["sq_err_share"] = _div(sq[m].sum(), sq.sum())
            row["mse"] = _div(sq[m].sum(), k * pix)
            row["psnr"] = float(10.0 * np.log10(1.0 / row["mse"])) if row["mse"] else None
            row["ssim"] = _div(ss[m].sum(), 3.0 * win_flat[m].sum())
        if bits is not None:
            row["bits_share"] = _div(cell_bits[m].sum(), cell_bits.sum())
            mm = m.reshape(n, ncell)
            row["bits_per_token"] = {name: _div((bits[:, i, :, 0] * mm).sum() / _LN2, (bits[:, i, :, 1] * mm).sum())
                                     for i, name in enumerate(LIKELIHOOD_STREAMS)}
        by_grain.append(row)
    deciles = None
    if ent is not None:
        idx, edges = decile_index(ent)
        deciles = {"edges": [float(e) for e in edges], "rows": []}
        for d in range(10):
            m = idx == d
            k = int(m.sum())
            deciles["rows"].append({"decile": d, "cells": k, "entropy": _div(ent[m].sum(), k),
                                    "sq_err": _div(sq[m].sum(), k) if sq is not None else None,
                                    "mse": _div(sq[m].sum(), k * pix) if sq is not None else None,
                                    "bits": _div(cell_bits[m].sum(), k) if cell_bits is not None else None,
                                    "fine_fraction": _div(float((g_flat[m] > 0).sum()), k)})
    pairs = {"entropy_error": (ent, sq), "entropy_bits": (ent, cell_bits), "bits_error": (cell_bits, sq)}
    corr = {}
    for name, (a, b) in pairs.items():
        if a is None or b is None:
            corr[name] = None
            continue
        corr[name] = {"pooled": spearman(a, b), "by_grain": [spearman(a[g_flat == g], b[g_flat == g]) for g in range(n_grains)]}
    cons = {"sq_err": None, "abs_err": None, "ssim": None, "nll": None, "counts_equal": None, "max": None}
    if recon is not None and ref_recon is not None:
        mse, l1, ssim = [np.asarray(v, dtype=np.float64).reshape(-1) for v in ref_recon]
        cons["sq_err"] = _rel_gap(recon[..., 0].sum(axis=(1, 2)) / (3.0 * h * w), mse)
        cons["abs_err"] = _rel_gap(recon[..., 1].sum(axis=(1, 2)) / (3.0 * h * w), l1)
        if win.sum() > 0:
            cons["ssim"] = _rel_gap(recon[..., 2].sum(axis=(1, 2)) / (3.0 * win.sum()), ssim)
    if bits is not None and ref_score is not None:
        ref_score = np.asarray(ref_score, dtype=np.float64).reshape(n, 4, 4)
        tot = bits.sum(axis=2) + outside
        cons["nll"] = _rel_gap(tot[:, :, 0], ref_score[:, :, 0])
        cons["counts_equal"] = bool(np.array_equal(tot[:, :, 1:], ref_score[:, :, 1:]))
    gaps = [cons[k] for k in ("sq_err", "abs_err", "ssim", "nll") if cons[k] is not None]
    cons["max"] = max(gaps) if gaps else None
    out = {"n_images": int(n), "grid": [int(hg), int(wg)], "cell_pixels": [int(h // hg), int(w // wg)], "by_grain": by_grain,
           "by_entropy_decile": deciles, "rank_correlation": corr, "consistency": cons}
    if bits is not None:
        out["outside_bits_share"] = _div(outside[:, :, 0].sum(), outside[:, :, 0].sum() + bits[:, :, :, 0].sum())
    return out


def cell_maps(h, w, grain, recon=None, entropy=None, bits=None, outside=None) -> dict:
    """the per-image arrays of a --maps file: sq_err / abs_err (cell sums) and ssim (cell MEAN over its windows, NaN for a cell without
    one) [N, hg, wg]; entropy, grain [N, hg, wg]; bits [N, 4, hg, wg] (nll sums / ln 2, axis 1 = LIKELIHOOD_STREAMS), tokens
    [N, 4, hg, wg]; outside [N, 4, 4] (dvq_nll_cell_sums' values: nats, tokens, top-1, top-5).  Absent maps are left out."""
    grain = np.asarray(grain, dtype=np.int64)
    n, hg, wg = grain.shape
    out = {"grain": grain, "image_size": np.array([h, w], dtype=np.int64)}
    if recon is not None:
        recon = np.asarray(recon, dtype=np.float64).reshape(n, hg, wg, 3)
        win = 3.0 * cell_window_counts(h, w, hg, wg)
        out["sq_err"], out["abs_err"] = recon[..., 0].copy(), recon[..., 1].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            out["ssim"] = np.where(win > 0, recon[..., 2] / win, np.nan)
    if entropy is not None:
        out["entropy"] = np.asarray(entropy, dtype=np.float64).reshape(n, hg, wg)
    if bits is not None:
        bits = np.asarray(bits, dtype=np.float64).reshape(n, 4, hg, wg, 4)
        out["bits"], out["tokens"] = bits[..., 0] / _LN2, bits[..., 1].copy()
        out["outside"] = np.asarray(outside, dtype=np.float64).reshape(n, 4, 4)
    return out


def save_cell_maps(path: str, maps: dict) -> None:
    if not path.endswith(".npz"):
        raise ValueError("--maps takes a .npz path")
    np.savez(path, **maps)


def load_cell_maps(path: str) -> dict:
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


class CellMeter:
    """Accumulates cell maps of evaluation batches on the device; nothing is copied to the host until summary().
    update_recon(x, rec, grain, entropy=None): error cells of the pair over the grain map's grid (dvq_recon_cells), the per-image
    figures of dvq_recon_metrics next to them, and the patch entropy at the cell size (the entropy kernel, whatever routes the model).
    update_bits(cells, outside, score=None, grain=None): Dualformer.score_cells' pair (+ score()'s block for the consistency figure);
    grain: only when no update_recon supplies it (token batches)."""

    def __init__(self, n_grains: int = 2, quantize_u8: bool = True):
        self.n_grains, self.quantize_u8 = int(n_grains), bool(quantize_u8)
        self.size = None
        self._ws = {}
        self._recon, self._ref, self._ent, self._grain, self._bits, self._out, self._score = [], [], [], [], [], [], []

    def _set_size(self, h, w):
        if self.size not in (None, (h, w)):
            raise ValueError("images of different sizes in one cell-map evaluation")
        self.size = (h, w)

    def update_recon(self, x, rec, grain, entropy=None):
        b, _, h, w = x.shape
        hg, wg = int(grain.shape[1]), int(grain.shape[2])
        if h % hg or w % wg or h // hg != w // wg:
            raise ValueError(f"a {hg} x {wg} grain map does not cut a {h} x {w} image into square cells")
        self._set_size(h, w)
        key = (b, h, w, hg, wg)
        if key not in self._ws:
            self._ws[key] = (K.recon_cells_workspace(b, h, w, hg, wg, x.device), K.recon_metrics_workspace(b, h, w, x.device))
        self._recon.append(K.recon_cells(x, rec, hg, wg, self.quantize_u8, self._ws[key][0]))
        if h >= 11 and w >= 11:
            self._ref.append(torch.stack(K.recon_metrics(x, rec, self.quantize_u8, self._ws[key][1]), dim=1))
        if entropy is None or tuple(entropy.shape) != (b, hg, wg):
            entropy = K.patch_entropy_gate(x, h // hg, None)[0]
        self._ent.append(entropy)
        self._grain.append(grain)

    def update_bits(self, cells, outside, score=None, grain=None, size=None):
        self._bits.append(cells)
        self._out.append(outside)
        if score is not None:
            self._score.append(score)
        if grain is not None:
            self._grain.append(grain)
        if size is not None:
            self._set_size(*size)

    def summary(self, maps: bool = False) -> dict:
        """the one host copy, then aggregate_cells; maps=True adds "maps" (cell_maps' dict of per-image arrays)"""
        if not self._grain:
            raise ValueError("CellMeter.summary(): no batch was added")

        def host(lst):
            return torch.cat(lst, dim=0).cpu().numpy() if lst else None
        grain, recon, ent, bits, outside = host(self._grain), host(self._recon), host(self._ent), host(self._bits), host(self._out)
        ref, score = host(self._ref), host(self._score)
        h, w = self.size
        if bits is not None and (bits.shape[0] != grain.shape[0] or bits.shape[2] != grain.shape[1] * grain.shape[2]):
            raise ValueError(f"bit maps {bits.shape} do not match the grain maps {grain.shape}")
        out = aggregate_cells(h, w, self.n_grains, grain, recon, ent, bits, outside,
                              ref_recon=(ref[:, 0], ref[:, 1], ref[:, 2]) if ref is not None else None, ref_score=score)
        if maps:
            out["maps"] = cell_maps(h, w, grain, recon, ent, bits, outside)
        return out


def evaluate_cells(model, batches, stage2=None, quantize_u8: bool = True, maps: bool = False) -> dict:
    """Where error and bits fall (docs/design/30-cell-maps.md).  model: a DQ-VAE, or None with stage2 (its frozen first stage is used);
    stage2: a Dualformer / ClassDualformer, or None (error maps only).  Per image batch: one model.ae_fwd(x, None) for the
    reconstruction and the grain map, the patch entropy at the cell size, and with stage2 one score_cells (+ one score: the per-image
    figure the cells are checked against).  Token batches ({"tokens": ...}) give bit maps only; their grain map is read off the fine
    stream's token counts.  Everything stays on the device until the summary.  Keys: aggregate_cells(), dtype; maps=True: "maps"."""
    if model is None:
        if stage2 is None:
            raise ValueError("evaluate_cells needs a model")
        model = stage2.first_stage_model
    model.eval()
    meter = CellMeter(getattr(model, "N_GRAINS", 2), quantize_u8=quantize_u8)
    with torch.no_grad():
        for batch in batches:
            if isinstance(batch, dict) and "tokens" in batch:
                if stage2 is None:
                    raise ValueError("token batches need a stage-2 model")
                tokens, c = stage2.get_tc(batch)
                cells, outside = stage2.score_cells_tokens(tokens, c)
                grain = (cells[:, 1, :, 1] > 0).long().view(-1, stage2.hw1, stage2.hw1)
                side = int(stage2.first_stage_model.encoder.resolution)
                meter.update_bits(cells, outside, stage2.score_tokens(tokens, c), grain=grain, size=(side, side))
                continue
            c = None
            if stage2 is not None and isinstance(batch, dict):
                x, c = stage2.get_xc(batch)
            else:
                x = batch[getattr(model, "image_key", "image")] if isinstance(batch, dict) else batch
            x = x.float().contiguous() if x.dtype != torch.float32 or not x.is_contiguous() else x
            out = model.ae_fwd(x, None)
            meter.update_recon(x, out["rec"], out["grain"], out["entropy"])
            if stage2 is not None:
                if c is None:
                    if stage2.cond_stage_key != stage2.first_stage_key:
                        raise ValueError(f"a conditional model needs dict batches with '{stage2.cond_stage_key}'")
                    c = x
                # one encode for both passes: the frozen first stage's float atomics may flip a code between two encodes
                _, z_out = stage2.encode_to_z(x)
                cells, outside = stage2._score_streams(z_out, c, cells=True)
                meter.update_bits(cells, outside, stage2._score_streams(z_out, c))
    s = meter.summary(maps=maps)
    s["dtype"] = dtype_name()
    return s


# ---- sample-set metrics on feature vectors (docs/design/32-sample-set-metrics.md) -----------------------------------------------------
SAMPLE_NOTES = {
    "dqvae": "feature space: the frozen DQ-VAE's pooled merged map; the values compare runs of this tree and are NOT the published FID / "
             "precision / recall (those are defined on Inception pool3 features)",
    "npy": "feature space: the caller's feature rows; with Inception pool3 rows these are the published quantities",
    "fd": "the Frechet term is biased upwards at small N (the covariance estimates' trace term): compare runs at equal N only",
}


def moments_from_sums(total, gram, n, shift=None) -> dict:
    """dvq_feat_moments' outputs (sum and upper-triangle Gram matrix of x - shift over n rows; arrays or tensors) ->
    {"n", "mean" fp64 [D], "cov" fp64 [D, D]}: the host mirrors the triangle; the covariance divides by n - 1"""
    to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)     # noqa: E731
    s, g, n = to_np(total).astype(np.float64).reshape(-1), to_np(gram).astype(np.float64), int(to_np(n).reshape(-1)[0])
    if n < 2:
        raise ValueError(f"a covariance needs at least 2 rows, got {n}")
    g = np.triu(g) + np.triu(g, 1).T
    mean = s / n
    cov = (g - n * np.outer(mean, mean)) / (n - 1)
    if shift is not None:
        mean = mean + to_np(shift).astype(np.float64).reshape(-1)
    return {"n": n, "mean": mean, "cov": cov}


def frechet_distance(moments_r: dict, moments_f: dict) -> float:
    """|mu_r - mu_f|^2 + tr S_r + tr S_f - 2 tr (S_r^1/2 S_f S_r^1/2)^1/2 in fp64 through two symmetric eigendecompositions (negative
    eigenvalues of either are rounding and clamp to 0, as do those of the product below D eps of its largest; the value is clamped at 0): stable on rank-deficient covariances, where the square root of the unsymmetric
    product S_r S_f is not"""
    mr, mf = np.asarray(moments_r["mean"], np.float64), np.asarray(moments_f["mean"], np.float64)
    sr, sf = np.asarray(moments_r["cov"], np.float64), np.asarray(moments_f["cov"], np.float64)
    w, v = np.linalg.eigh((sr + sr.T) * 0.5)
    root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = root @ ((sf + sf.T) * 0.5) @ root
    ev = np.linalg.eigvalsh((m + m.T) * 0.5)
    # rank-deficient covariances (fewer rows than columns): the exact zeros come out as +-D eps |M|, and the square roots of the positive
    # half would take ~1e-7 tr S off the value (FD(X, X) < 0).  Eigenvalues below D eps max(ev) are those zeros
    ev = np.where(ev > ev.size * np.finfo(np.float64).eps * max(float(ev.max()), 0.0), ev, 0.0)
    d = mr - mf
    return max(float(d @ d + np.trace(sr) + np.trace(sf) - 2.0 * np.sqrt(ev).sum()), 0.0)


def _finite_features(name, x):
    if not torch.is_tensor(x) or x.dim() != 2 or not x.is_floating_point():
        raise TypeError(f"{name}: expected a floating-point [N, D] device tensor")
    bad = int((~torch.isfinite(x).all(dim=1)).sum())
    if bad:
        raise ValueError(f"{name}: {bad} of {x.shape[0]} feature rows hold a non-finite value")


def sample_set_metrics(real, fake, k: int = 5, neighbors: int = 0) -> dict:
    """Fidelity and diversity of a generated set against a real one, on device feature tensors real [Nr, D], fake [Nf, D]:
    fd (Frechet distance of the two Gaussians), improved precision / recall, density / coverage, all with k-th-neighbour radii.
    Both sets are centred on the REAL set's mean and cast to fp32 (part of the definition: it keeps dvq_pair_scan's GEMM-form distance
    accurate); two moment passes and four scans (R|R, F|F, F|R, R|F) run on the device, the reduction on the host in integers / fp64.
    neighbors > 0 adds "neighbor_idx" int64 [Nf, neighbors] and "neighbor_dist" fp32 (squared, centred fp32 features): each fake's
    nearest reals -- the memorisation check, from the F|R scan."""
    _finite_features("real", real)
    _finite_features("fake", fake)
    k, neighbors = int(k), int(neighbors)
    nr, d = int(real.shape[0]), int(real.shape[1])
    nf = int(fake.shape[0])
    if fake.shape[1] != d:
        raise ValueError(f"real features have {d} columns, fake {fake.shape[1]}")
    if not 1 <= k <= 16 or not 0 <= neighbors <= 16:
        raise ValueError(f"k={k} / neighbors={neighbors}: the scan keeps 1..16 neighbours")
    if min(nr, nf) <= k:
        raise ValueError(f"k={k} needs more than k rows in both sets (real {nr}, fake {nf})")
    mean = real.double().mean(dim=0)
    xr = (real.double() - mean).float().contiguous()
    xf = (fake.double() - mean).float().contiguous()
    zero = torch.zeros(d, dtype=torch.float32, device=xr.device)
    mom_r, mom_f = K.feat_moments(xr, zero), K.feat_moments(xf, zero)
    rad_r = K.pair_scan(xr, xr, k, exclude_diag=True)[0][:, k - 1].contiguous()
    rad_f = K.pair_scan(xf, xf, k, exclude_diag=True)[0][:, k - 1].contiguous()
    d_fr, i_fr, c_fr = K.pair_scan(xf, xr, max(neighbors, 1), rad2_b=rad_r)
    d_rf, _, c_rf = K.pair_scan(xr, xf, 1, rad2_b=rad_f)
    c_fr, c_rf = c_fr.cpu().numpy(), c_rf.cpu().numpy()
    out = {
        "fd": frechet_distance(moments_from_sums(*mom_r), moments_from_sums(*mom_f)),
        "precision": float(np.mean(c_fr > 0)),
        "recall": float(np.mean(c_rf > 0)),
        "density": float(int(c_fr.sum()) / (k * nf)),
        "coverage": float(np.mean(d_rf[:, 0].cpu().numpy() <= rad_r.cpu().numpy())),
        "k": k, "n_real": nr, "n_fake": nf, "dim": d,
    }
    if neighbors > 0:
        out["neighbor_idx"], out["neighbor_dist"] = i_fr.cpu().numpy(), d_fr.cpu().numpy()
    return out


def evaluate_samples(model, real_batches, fake_batches, k: int = 5, grid: int = 2, neighbors: int = 0) -> dict:
    """sample_set_metrics in the frozen DQ-VAE's own feature space: both image streams (NCHW [-1, 1] batches, or dicts holding one
    under model.image_key) go through model.pooled_features(x, grid); the features stay on the device (50 000 x 1024 fp32: 200 MB
    per set).  Keys: sample_set_metrics(), plus grid, features, dtype and the notes."""
    def features(batches):
        rows = []
        for batch in batches:
            x = batch[getattr(model, "image_key", "image")] if isinstance(batch, dict) else batch
            rows.append(model.pooled_features(x, grid))
        if not rows:
            raise ValueError("evaluate_samples: an image stream is empty")
        return torch.cat(rows, dim=0)

    s = sample_set_metrics(features(real_batches), features(fake_batches), k=k, neighbors=neighbors)
    s.update(grid=int(grid), features="dqvae", dtype=dtype_name(), note=SAMPLE_NOTES["dqvae"], fd_note=SAMPLE_NOTES["fd"])
    return s


def checkpoint_state_dict(ckpt, use_ema: bool = False):
    """the model state dict of a checkpoint: ckpt["state_dict"] of a Lightning-style file, or the bare dict itself.  use_ema: a COPY
    with the averaged weights ckpt["ema"]["state_dict"] (Trainer(ema_decay=...), docs/design/20-weight-ema.md) laid over it -- exactly
    the listed names are replaced, everything else (buffers, forward-updated codebooks, frozen parts) stays; the input is not
    modified.  KeyError when the checkpoint has no "ema" key, or an averaged tensor has no counterpart of its name and shape."""
    sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    if not use_ema:
        return sd
    ema = ckpt.get("ema") if "state_dict" in ckpt else None
    if not isinstance(ema, dict) or "state_dict" not in ema:
        raise KeyError("checkpoint has no \"ema\" key: it was written without --ema_decay (or is an export_ema.py output, whose "
                       "state_dict already is the averaged model)")
    out = dict(sd)
    for name, t in ema["state_dict"].items():
        if name not in sd:
            raise KeyError(f"EMA tensor {name!r} has no counterpart in the checkpoint's state_dict")
        if tuple(t.shape) != tuple(sd[name].shape):
            raise KeyError(f"EMA tensor {name!r} has shape {tuple(t.shape)}, the state_dict's has {tuple(sd[name].shape)}")
        out[name] = t
    return out


def load_checkpoint_state_dict(model_path: str, use_ema: bool = False):
    """checkpoint_state_dict of a file (loaded to the CPU)"""
    return checkpoint_state_dict(torch.load(model_path, map_location="cpu"), use_ema=use_ema)


def load_stage2_model(yaml_path: str, model_path: str = "", device="cuda", seed: int = 0, use_ema: bool = False):
    """the Dualformer of a stage-2 YAML, weights from a checkpoint when given (use_ema: its averaged weights), in eval mode on
    `device` (seeded initialisation, like load_model).  Returns (model, image size of its first stage)."""
    from . import config as cfg
    conf = cfg.load_yaml(yaml_path)
    torch.manual_seed(seed)
    model = cfg.instantiate_from_config(conf.model)
    if not hasattr(model, "score"):
        raise ValueError(f"{yaml_path}: not a stage-2 (DQ-Transformer) model")
    if model_path:
        model.load_state_dict(load_checkpoint_state_dict(model_path, use_ema), strict=False)
    fs = conf.model.params.first_stage_config.params
    size = fs.get("image_size") or fs.encoderconfig.params.resolution
    return model.eval().to(device), int(size)


def read_labels(path: str):
    """int64 class labels, one per image in image order: a .npy array, or a text file of whitespace / comma separated integers"""
    if path.endswith(".npy"):
        lab = np.load(path)
    else:
        with open(path, "r", encoding="utf-8") as f:
            lab = np.array([int(v) for v in f.read().replace(",", " ").split()], dtype=np.int64)
    lab = np.asarray(lab)
    if lab.ndim != 1 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"{path}: expected a 1-d integer array of labels, got {lab.dtype} {lab.shape}")
    return lab.astype(np.int64)


# ---- inputs of the evaluation scripts (scripts/tools/eval_reconstruction.py, codebook_usage_dqvae.py) ---------------------------------
IMAGE_EXTS = (".jpeg", ".jpg", ".png", ".bmp", ".webp")


def folder_dataset(root: str, limit: int | None = None):
    """data.ImageFolder over <root>/<class dir>/<image>, or the sorted image files of `root` itself when it has no subdirectory"""
    import os

    from . import data
    if any(os.path.isdir(os.path.join(root, d)) for d in os.listdir(root)):
        ds = data.ImageFolder(root, limit=limit)
    else:
        files = sorted(os.path.join(root, f) for f in os.listdir(root) if f.lower().endswith(IMAGE_EXTS))
        ds = data.ImagePaths(files[:limit] if limit else files)
    if len(ds) == 0:
        raise FileNotFoundError(f"no images under {root}")
    return ds


def image_batches(batch_size: int, size: int, device, images: str | None = None, synthetic: int = 0, limit: int | None = None,
                  seed: int = 2021, num_workers: int = 8, device_decode: bool = False, device_png: bool = False):
    """NCHW fp32 [b,3,size,size] device batches in [-1, 1], streamed (never the whole set in host memory):
    synthetic > 0: synth.half_flat_images per batch; images = *.npy: memory-mapped [N,3,H,W] fp32, read per batch; images = folder:
    decoded on host threads, transformed on the GPU (data.GpuBatchLoader, the eval transform: Resize + CenterCrop); device_decode: its
    JPEG files through the device decoder (docs/design/23-device-jpeg.md) -- the same pixels, less host work per image; device_png: its
    PNG files likewise (docs/design/29-device-png.md)"""
    import numpy as np

    from . import data, synth
    if synthetic > 0:
        n = min(synthetic, limit) if limit else synthetic
        for i in range(0, n, batch_size):
            yield torch.from_numpy(synth.half_flat_images(min(batch_size, n - i), size, seed=seed + i)).to(device)
    elif images is not None and images.endswith(".npy"):
        a = np.load(images, mmap_mode="r")
        if a.ndim != 4 or a.shape[1] != 3:
            raise ValueError(f"{images}: expected [N,3,H,W], got {a.shape}")
        n = min(a.shape[0], limit) if limit else a.shape[0]
        for i in range(0, n, batch_size):
            yield torch.from_numpy(np.array(a[i:min(i + batch_size, n)], dtype=np.float32)).to(device)     # a writable copy of the slice
    elif images is not None:
        loader = data.GpuBatchLoader(folder_dataset(images, limit), batch_size, device, size=size, shuffle=False,
                                     num_workers=num_workers, drop_last=False, device_decode=device_decode, device_png=device_png)
        for b in loader:
            yield b["image"]
    else:
        raise ValueError("no image source: give images=<folder|.npy> or synthetic=N")


def load_model(yaml_path: str, model_path: str = "", device="cuda", seed: int = 0, use_ema: bool = False):
    """the model of a stage-1 YAML (config.instantiate_from_config), weights from a checkpoint ({"state_dict": ...} or a bare state
    dict) when given -- with use_ema its averaged weights (checkpoint_state_dict) --, in eval mode on `device`.  The initialisation is seeded, so that runs without a checkpoint evaluate the same
    random weights.  Returns (model, image size)."""
    from . import config as cfg
    conf = cfg.load_yaml(yaml_path)
    torch.manual_seed(seed)
    model = cfg.instantiate_from_config(conf.model)
    if model_path:
        model.load_state_dict(load_checkpoint_state_dict(model_path, use_ema))
    params = conf.model.params
    size = int(params.get("image_size", 256)) if hasattr(params, "get") else 256
    return model.eval().to(device), size


def add_eval_args(ap) -> None:
    """the flags both evaluation scripts take: the reference tool's (--yaml_path --model_path --batch_size --dataset_type
    --codebook_size) and the image source / compute dtype"""
    ap.add_argument("--yaml_path", type=str, required=True)
    ap.add_argument("--model_path", type=str, default="", help="checkpoint; empty: the YAML's freshly initialised weights")
    ap.add_argument("--use_ema", action="store_true",
                    help="evaluate the averaged weights stored under the checkpoint's \"ema\" key (train.py --ema_decay)")
    ap.add_argument("--batch_size", type=int, default=100)
    ap.add_argument("--dataset_type", type=str, default="ffhq", choices=["ffhq", "imagenet"],
                    help="imagenet: $DVQ_IMAGENET_ROOT/val; ffhq needs --images (no FFHQ loader)")
    ap.add_argument("--codebook_size", type=int, default=None, help="denominator of the usage line (default: the model's K)")
    ap.add_argument("--images", type=str, default=None, help="folder of images or a [N,3,H,W] fp32 .npy in [-1, 1]")
    ap.add_argument("--synthetic", type=int, default=0, help="N half-flat synthetic images instead of a dataset")
    ap.add_argument("--limit", type=int, default=None, help="evaluate the first N images only")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp32x3"])
    ap.add_argument("--device_jpeg", action="store_true",
                    help="image folders: decode JPEG files on the GPU after a Huffman pass on host threads (same pixels as PIL; other "
                         "files are decoded by PIL as before)")
    ap.add_argument("--device_png", action="store_true",
                    help="image folders: un-filter PNG files on the GPU after inflating them on host threads (same pixels as PIL; palette, "
                         "16-bit and interlaced files are decoded by PIL as before)")


def image_source(opt, ap) -> str | None:
    """the folder / .npy the flags name (None for --synthetic); calls ap.error (exit 2) before any model or device work"""
    if opt.synthetic > 0:
        return None
    if opt.images:
        return opt.images
    if opt.dataset_type == "imagenet":
        from .data import _imagenet_root
        try:
            return _imagenet_root("val")
        except FileNotFoundError as e:
            ap.error(str(e))
    ap.error(f"--dataset_type {opt.dataset_type}: this repository has no {opt.dataset_type.upper()} loader; "
             "give --images <folder|.npy> (or --synthetic N)")
