#!/usr/bin/env python3
"""Metrics of a SET of generated images against a set of real ones: Frechet distance, improved precision / recall (Kynkaanniemi et al.
2019) and density / coverage (Naeem et al. 2020) with k-th-neighbour radii (docs/design/32-sample-set-metrics.md).  Prints ONE JSON
line (also written to --json).

--real / --fake each name an image folder, a sampler .npz (arr_0 uint8 NHWC, what sample_dynamic_class.py --npz writes) or, with
--features npy, a .npy of feature rows [N, D] extracted elsewhere (no model is loaded then; with Inception pool3 rows the values are
the published quantities).  --features dqvae (default) uses the frozen DQ-VAE's own pooled encoder features: a yardstick for
comparing sampling settings and checkpoints of this tree, NOT the published FID.

    python scripts/tools/eval_samples.py --yaml_path configs/stage1/dqvae-entropy-dual-r05_imagenet.yml --model_path last.ckpt \\
        --real /data/imagenet/val --fake samples.npz --limit 50000 --neighbors 3 --neighbors_out nearest.npz
    python scripts/tools/eval_samples.py --features npy --real real_pool3.npy --fake fake_pool3.npy
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

KEYS = ("fd", "precision", "recall", "density", "coverage", "k", "n_real", "n_fake", "dim")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--real", type=str, required=True, help="image folder, sampler .npz, or (--features npy) a [N, D] .npy")
    ap.add_argument("--fake", type=str, required=True, help="the same kinds, for the generated set")
    ap.add_argument("--features", default="dqvae", choices=["dqvae", "npy"])
    ap.add_argument("--yaml_path", type=str, default="", help="--features dqvae: the stage-1 YAML")
    ap.add_argument("--model_path", type=str, default="", help="checkpoint; empty: the YAML's freshly initialised weights")
    ap.add_argument("--use_ema", action="store_true", help="the averaged weights under the checkpoint's \"ema\" key")
    ap.add_argument("--grid", type=int, default=2, help="--features dqvae: pool the merged map onto grid x grid cells")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp32x3"])
    ap.add_argument("--batch_size", type=int, default=100)
    ap.add_argument("--k", type=int, default=5, help="neighbour rank of the radii (1..16)")
    ap.add_argument("--limit", type=int, default=None, help="use the first N items of each set only")
    ap.add_argument("--neighbors", type=int, default=0, help="K > 0: record each fake's K nearest reals (memorisation check)")
    ap.add_argument("--neighbors_out", type=str, default="", help="the .npz that receives idx [Nf, K] and dist [Nf, K] (squared)")
    ap.add_argument("--device_jpeg", action="store_true", help="image folders: decode JPEG files on the GPU")
    ap.add_argument("--device_png", action="store_true", help="image folders: un-filter PNG files on the GPU")
    ap.add_argument("--json", type=str, default="", help="also write the line to this file")
    opt = ap.parse_args(argv)
    if not 1 <= opt.k <= 16 or not 0 <= opt.neighbors <= 16:
        ap.error("--k must be in 1..16 and --neighbors in 0..16")
    if bool(opt.neighbors) != bool(opt.neighbors_out):
        ap.error("--neighbors K and --neighbors_out F.npz go together")
    if opt.features == "npy":
        for name in ("real", "fake"):
            if not getattr(opt, name).endswith(".npy"):
                ap.error(f"--features npy: --{name} must be a .npy of feature rows")
    elif not opt.yaml_path:
        ap.error("--features dqvae needs --yaml_path")
    return opt


def load_features(path, limit=None):
    """[N, D] feature rows of a .npy (first `limit` rows), as a float array"""
    import numpy as np
    a = np.load(path, mmap_mode="r")
    if a.ndim != 2 or a.dtype.kind != "f":
        raise ValueError(f"{path}: expected a floating-point [N, D] array, got {a.dtype} {a.shape}")
    return np.array(a[:limit] if limit else a)


def npz_batches(path, batch_size, size, device, limit=None):
    """a sampler .npz (arr_0 uint8 NHWC) as NCHW fp32 device batches in [-1, 1]"""
    import numpy as np
    import torch
    a = np.load(path)["arr_0"]
    if a.ndim != 4 or a.shape[3] != 3 or a.dtype != np.uint8:
        raise ValueError(f"{path}: expected arr_0 uint8 [N, H, W, 3], got {a.dtype} {a.shape}")
    if a.shape[1] != size or a.shape[2] != size:
        raise ValueError(f"{path}: {a.shape[1]} x {a.shape[2]} images, the model takes {size} x {size}")
    n = min(a.shape[0], limit) if limit else a.shape[0]
    for i in range(0, n, batch_size):
        x = torch.from_numpy(a[i:min(i + batch_size, n)]).to(device)
        yield (x.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()


def record(opt, metrics):
    """the JSON line: the metrics, the feature space they were computed in and the two caveats"""
    from dynamicvectorquantization_amd.evaluate import SAMPLE_NOTES
    line = {key: metrics[key] for key in KEYS}
    line.update(features=opt.features, note=SAMPLE_NOTES[opt.features], fd_note=SAMPLE_NOTES["fd"], real=opt.real, fake=opt.fake)
    if opt.features == "dqvae":
        line.update(grid=metrics["grid"], dtype=metrics["dtype"], yaml_path=opt.yaml_path, model_path=opt.model_path, use_ema=bool(opt.use_ema))
    if opt.neighbors:
        line.update(neighbors=opt.neighbors, neighbors_out=opt.neighbors_out)
    return line


def main(argv=None):
    opt = parse_args(argv)
    import numpy as np
    import torch

    from dynamicvectorquantization_amd import evaluate as E
    if opt.features == "npy":
        real, fake = load_features(opt.real, opt.limit), load_features(opt.fake, opt.limit)
        if not torch.cuda.is_available():
            raise SystemExit("eval_samples.py: the scans run on the GPU (libdvq_hip has no CPU path); no device was found")
        m = E.sample_set_metrics(torch.from_numpy(real).to("cuda"), torch.from_numpy(fake).to("cuda"), k=opt.k, neighbors=opt.neighbors)
    else:
        from dynamicvectorquantization_amd import runtime as rt
        rt.set_compute_dtype(opt.dtype)
        model, size = E.load_model(opt.yaml_path, opt.model_path, "cuda", use_ema=opt.use_ema)

        def batches(path):
            if path.endswith(".npz"):
                return npz_batches(path, opt.batch_size, size, "cuda", opt.limit)
            return E.image_batches(opt.batch_size, size, "cuda", path, 0, opt.limit, device_decode=opt.device_jpeg, device_png=opt.device_png)

        m = E.evaluate_samples(model, batches(opt.real), batches(opt.fake), k=opt.k, grid=opt.grid, neighbors=opt.neighbors)
    if opt.neighbors:
        np.savez(opt.neighbors_out, idx=m["neighbor_idx"], dist=m["neighbor_dist"])
    line = json.dumps(record(opt, m))
    if opt.json:
        with open(opt.json, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
