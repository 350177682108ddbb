"""Reconstruction evaluation of a DQ-VAE: PSNR / SSIM / L1 (+ LPIPS when pretrained weights exist), codebook usage, perplexity
and tokens per image (docs/design/13-evaluation.md).

  * ReconstructionMeter      accumulates batches on the device (csrc/metrics.hip: dvq_recon_metrics, dvq_code_histogram); nothing is
                             copied to the host until summary(), which aggregates in fp64
  * aggregate                the host aggregation of per-image values and code counts (pure numpy: testable without a GPU)
  * evaluate_reconstruction  one model.ae_fwd(x, None) per batch in eval mode under no_grad: reconstruction, code map and grain map
                             of entropy-routed and feature-routed dual / triple grain models from one pass; no EMA update

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
    cbk = model.quantize.codebook
    meter = ReconstructionMeter(cbk.n_embed, model.N_GRAINS, quantize_u8=quantize_u8)
    lp_mod = _lpips_module(lpips, cbk.weight.device)
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
                  seed: int = 2021, num_workers: int = 8):
    """NCHW fp32 [b,3,size,size] device batches in [-1, 1], streamed (never the whole set in host memory):
    synthetic > 0: synth.half_flat_images per batch; images = *.npy: memory-mapped [N,3,H,W] fp32, read per batch; images = folder:
    decoded on host threads, transformed on the GPU (data.GpuBatchLoader, the eval transform: Resize + CenterCrop)"""
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
                                     num_workers=num_workers, drop_last=False)
        for b in loader:
            yield b["image"]
    else:
        raise ValueError("no image source: give images=<folder|.npy> or synthetic=N")


def load_model(yaml_path: str, model_path: str = "", device="cuda", seed: int = 0):
    """the model of a stage-1 YAML (config.instantiate_from_config), weights from a checkpoint ({"state_dict": ...} or a bare state
    dict) when given, in eval mode on `device`.  The initialisation is seeded, so that runs without a checkpoint evaluate the same
    random weights.  Returns (model, image size)."""
    from . import config as cfg
    conf = cfg.load_yaml(yaml_path)
    torch.manual_seed(seed)
    model = cfg.instantiate_from_config(conf.model)
    if model_path:
        sd = torch.load(model_path, map_location="cpu")
        model.load_state_dict(sd["state_dict"] if "state_dict" in sd else sd)
    params = conf.model.params
    size = int(params.get("image_size", 256)) if hasattr(params, "get") else 256
    return model.eval().to(device), size


def add_eval_args(ap) -> None:
    """the flags both evaluation scripts take: the reference tool's (--yaml_path --model_path --batch_size --dataset_type
    --codebook_size) and the image source / compute dtype"""
    ap.add_argument("--yaml_path", type=str, required=True)
    ap.add_argument("--model_path", type=str, default="", help="checkpoint; empty: the YAML's freshly initialised weights")
    ap.add_argument("--batch_size", type=int, default=100)
    ap.add_argument("--dataset_type", type=str, default="ffhq", choices=["ffhq", "imagenet"],
                    help="imagenet: $DVQ_IMAGENET_ROOT/val; ffhq needs --images (no FFHQ loader)")
    ap.add_argument("--codebook_size", type=int, default=None, help="denominator of the usage line (default: the model's K)")
    ap.add_argument("--images", type=str, default=None, help="folder of images or a [N,3,H,W] fp32 .npy in [-1, 1]")
    ap.add_argument("--synthetic", type=int, default=0, help="N half-flat synthetic images instead of a dataset")
    ap.add_argument("--limit", type=int, default=None, help="evaluate the first N images only")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp32x3"])


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
