#!/usr/bin/env python3
"""Reconstruction quality and codebook usage of a (trained) DQ-VAE: PSNR, SSIM, L1, LPIPS (only with pretrained VGG16 / LPIPS
weights), codes used, perplexity, grain fractions and tokens per image (docs/design/13-evaluation.md).  Prints ONE JSON line with the
summary (also written to --json).  --dump_dir writes every reconstruction as an 8-bit PNG -- the same quantisation the metrics use
with --quantize_u8 -- for an external rFID tool.

    python scripts/tools/eval_reconstruction.py --yaml_path configs/stage1/dqvae-entropy-dual-r05_imagenet.yml \\
        --model_path last.ckpt --dataset_type imagenet --batch_size 64 --dtype fp32 --json eval.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from dynamicvectorquantization_amd import evaluate as E  # noqa: E402


def to_u8(rec):
    """NCHW [-1, 1] -> NHWC uint8: floor(clamp(v * 0.5 + 0.5, 0, 1) * 255 + 0.5), in fp64 like dvq_recon_metrics"""
    import numpy as np
    v = np.clip(rec.astype(np.float64) * 0.5 + 0.5, 0.0, 1.0)
    return np.floor(v * 255.0 + 0.5).astype(np.uint8).transpose(0, 2, 3, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    E.add_eval_args(ap)
    ap.add_argument("--quantize_u8", action=argparse.BooleanOptionalAction, default=True,
                    help="metrics on 8-bit quantised images (what a saved PNG holds); --no_quantize_u8: on the fp32 values")
    ap.add_argument("--json", type=str, default="", help="also write the summary to this file")
    ap.add_argument("--dump_dir", type=str, default="", help="write the reconstructions as uint8 PNGs (000000.png, ...)")
    opt, _ = ap.parse_known_args()
    source = E.image_source(opt, ap)
    from dynamicvectorquantization_amd import runtime as rt
    rt.set_compute_dtype(opt.dtype)
    model, size = E.load_model(opt.yaml_path, opt.model_path, "cuda", use_ema=opt.use_ema)
    on_batch = None
    if opt.dump_dir:
        from PIL import Image
        os.makedirs(opt.dump_dir, exist_ok=True)
        n_done = [0]

        def on_batch(x, out):        # one device-to-host copy per batch, only when dumping
            for img in to_u8(out["rec"].cpu().numpy()):
                Image.fromarray(img, "RGB").save(os.path.join(opt.dump_dir, f"{n_done[0]:06d}.png"))
                n_done[0] += 1

    s = E.evaluate_reconstruction(model, E.image_batches(opt.batch_size, size, "cuda", source, opt.synthetic, opt.limit, device_decode=opt.device_jpeg, device_png=opt.device_png),
                                  quantize_u8=opt.quantize_u8, on_batch=on_batch)
    line = json.dumps(s)
    if opt.json:
        with open(opt.json, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
