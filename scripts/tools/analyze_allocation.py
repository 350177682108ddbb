#!/usr/bin/env python3
"""Where an image's reconstruction error and its bits fall: per-cell maps of a DQ-VAE / DQ-Transformer, aggregated by grain, by
patch-entropy decile and as rank correlations (docs/design/30-cell-maps.md).  Prints ONE JSON line with the blocks by_grain,
by_entropy_decile, rank_correlation and consistency (also written to --json).

    # error maps only: a stage-1 YAML + checkpoint
    python scripts/tools/analyze_allocation.py --yaml_path configs/stage1/dqvae-entropy-dual-r05_imagenet.yml --model_path vae.ckpt \\
        --dataset_type imagenet --batch_size 32
    # error and bit maps: a stage-2 YAML + checkpoint (its frozen first stage reconstructs)
    python scripts/tools/analyze_allocation.py --yaml_path configs/stage2/uncond_imagenet_p6c18.yml --model_path last.ckpt \\
        --dataset_type imagenet --batch_size 32 --maps maps.npz

--tokens DIR analyses a token set (scripts/tools/tokenize_dataset.py) with a stage-2 model: bit maps only, no first stage.
--maps F.npz writes the per-image arrays sq_err, abs_err, ssim, entropy, grain, bits[4], tokens[4], outside (evaluate.cell_maps).
A class-conditional model needs --labels (or the labels stored in the token set).

The tables describe an allocation, they do not rank routers: error and bits are measured AFTER the allocation, and a fine cell's lower
error is partly an effect of being fine.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from dynamicvectorquantization_amd import evaluate as E  # noqa: E402


def get_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    E.add_eval_args(ap)
    ap.add_argument("--labels", type=str, default="", help="class labels of a class-conditional model: .npy or text file, image order")
    ap.add_argument("--json", type=str, default="", help="also write the summary to this file")
    ap.add_argument("--maps", type=str, default="", help="write the per-image cell maps to this .npz")
    ap.add_argument("--tokens", type=str, default="", help="analyse this token set instead of images (bit maps only)")
    ap.add_argument("--view", type=int, default=0, help="--tokens: the stored view of every image to score")
    ap.add_argument("--no_quantize_u8", action="store_true", help="error on the float images instead of their 8-bit rounding")
    return ap


def is_stage2(yaml_path):
    from dynamicvectorquantization_amd import config as cfg
    params = cfg.load_yaml(yaml_path).model.params
    return "first_stage_config" in params


def main():
    ap = get_parser()
    opt, _ = ap.parse_known_args()
    if opt.maps and not opt.maps.endswith(".npz"):
        ap.error("--maps takes a .npz path")
    stage2 = is_stage2(opt.yaml_path)
    if opt.tokens and not stage2:
        ap.error("--tokens needs a stage-2 YAML")
    source = None if opt.tokens else E.image_source(opt, ap)
    labels = None
    if opt.labels:
        try:
            labels = E.read_labels(opt.labels)
        except (OSError, ValueError) as e:
            ap.error(f"--labels: {e}")
    from dynamicvectorquantization_amd import runtime as rt
    rt.set_compute_dtype(opt.dtype)
    if stage2:
        s2, size = E.load_stage2_model(opt.yaml_path, opt.model_path, "cuda", use_ema=opt.use_ema)
        model = None
    else:
        model, size = E.load_model(opt.yaml_path, opt.model_path, "cuda", use_ema=opt.use_ema)
        s2 = None
    if opt.tokens:
        from eval_likelihood import token_batches
        from dynamicvectorquantization_amd import tokens as T
        ds = T.TokenShardDataset(opt.tokens)
        ds.check_model(s2)
        if not 0 <= opt.view < ds.n_views:
            ap.error(f"--view {opt.view}: {opt.tokens} stores {ds.n_views} views per image")
        loader = T.TokenBatchLoader(ds, opt.batch_size, "cuda", s2.permuter, shuffle=False, drop_last=False, view=opt.view)
        batches = token_batches(loader, opt.limit, s2.cond_stage_key if s2.cond_stage_key != s2.first_stage_key else None, ap)
    else:
        batches = E.image_batches(opt.batch_size, size, "cuda", source, opt.synthetic, opt.limit, device_decode=opt.device_jpeg,
                                  device_png=opt.device_png)
        if s2 is not None and s2.cond_stage_key != s2.first_stage_key:
            from eval_likelihood import labelled_batches
            if labels is None:
                ap.error(f"{opt.yaml_path} is class-conditional: give --labels")
            batches = labelled_batches(batches, labels, s2.cond_stage_key)
    s = E.evaluate_cells(model, batches, stage2=s2, quantize_u8=not opt.no_quantize_u8, maps=bool(opt.maps))
    if opt.maps:
        E.save_cell_maps(opt.maps, s.pop("maps"))
    line = json.dumps(s)
    if opt.json:
        with open(opt.json, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
