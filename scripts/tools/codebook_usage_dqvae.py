#!/usr/bin/env python3
"""Codebook usage of a (trained) DQ-VAE -- the reference's scripts/tools/codebook_usage_dqvae.py on the HIP path.

Same flags (--yaml_path --model_path --batch_size --dataset_type --codebook_size) and the same two output lines: the number of codes
used over the whole set, then `usage:  <1 - used / codebook_size>` -- which, as in the reference, is the UNUSED fraction of the
codebook.  The codes are counted on the device (dvq_code_histogram: one token per grain cell position, so a coarse cell counts
once) from one autoencoder pass per batch.  Images come from --images (folder or .npy), --synthetic N, or
--dataset_type imagenet ($DVQ_IMAGENET_ROOT/val); there is no FFHQ loader, so --dataset_type ffhq needs --images.

    python scripts/tools/codebook_usage_dqvae.py --yaml_path configs/stage1/dqvae-entropy-dual-r05_imagenet.yml \\
        --model_path last.ckpt --dataset_type imagenet --batch_size 64
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from dynamicvectorquantization_amd import evaluate as E  # noqa: E402
from dynamicvectorquantization_amd.quantize import codebook_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    E.add_eval_args(ap)
    opt, _ = ap.parse_known_args()
    source = E.image_source(opt, ap)
    from dynamicvectorquantization_amd import runtime as rt
    rt.set_compute_dtype(opt.dtype)
    model, size = E.load_model(opt.yaml_path, opt.model_path, "cuda", use_ema=opt.use_ema)
    k = codebook_of(model.quantize)[1]
    if opt.codebook_size is not None and opt.codebook_size != k:
        print(f"warning: --codebook_size {opt.codebook_size} differs from the model's {k} codes", file=sys.stderr)
    s = E.evaluate_reconstruction(model, E.image_batches(opt.batch_size, size, "cuda", source, opt.synthetic, opt.limit, device_decode=opt.device_jpeg, device_png=opt.device_png), lpips=False)
    print(s["codes_used"])
    print("usage: ", 1 - s["codes_used"] / (opt.codebook_size or k))


if __name__ == "__main__":
    main()
