#!/usr/bin/env python3
"""Teacher-forced likelihood of images under a (trained) DQ-Transformer: per token stream (coarse / fine content, coarse / fine
position) nats per token, perplexity, top-1 / top-5 accuracy and tokens per image; in total nats and bits per image, bits per pixel,
and the weighted validation loss recomputed from the sums (docs/design/15-likelihood.md).  Prints ONE JSON line with the summary
(also written to --json).  --per_image writes the [N, 4, 4] array of per-image stream sums (nll in nats, tokens, top-1, top-5 hits).

    python scripts/tools/eval_likelihood.py --yaml_path configs/stage2/uncond_imagenet_p6c18.yml --model_path last.ckpt \\
        --dataset_type imagenet --batch_size 32 --json likelihood.json --per_image likelihood.npy

A class-conditional model needs --labels: a .npy or text file with one integer label per image, in image order.

--tokens DIR scores a token set (scripts/tools/tokenize_dataset.py) instead of images: one stored view per image (--view K), in stored
order, without the first stage; a class-conditional model takes the labels stored in the set.  Same JSON, same --per_image file.
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
    ap.add_argument("--per_image", type=str, default="", help="write the per-image [N,4,4] fp64 sums to this .npy")
    ap.add_argument("--tokens", type=str, default="", help="score this token set instead of images")
    ap.add_argument("--view", type=int, default=0, help="--tokens: the stored view of every image to score")
    return ap


def labelled_batches(images, labels, key):
    """image batches -> dict batches carrying the matching slice of `labels` (int64 numpy) under `key`"""
    import torch
    i = 0
    for x in images:
        b = int(x.shape[0])
        if i + b > labels.shape[0]:
            raise SystemExit(f"--labels holds {labels.shape[0]} labels, the images need at least {i + b}")
        yield {"image": x, key: torch.from_numpy(labels[i:i + b]).to(x.device)}
        i += b


def token_batches(loader, limit, label_key, ap):
    """the loader's batches, cut at --limit images; a class-conditional model needs the labels stored in the set"""
    n = 0
    for b in loader:
        if label_key is not None and label_key not in b:
            ap.error("the model is class-conditional and this token set stores no labels")
        k = len(b["n_tokens"])
        if limit and n + k > limit:
            k = limit - n
            if k <= 0:
                return
            b = dict(b, tokens={key: v[:k] for key, v in b["tokens"].items()}, n_tokens=b["n_tokens"][:k],
                     **({label_key: b[label_key][:k]} if label_key is not None else {}))
        n += k
        yield b


def main():
    ap = get_parser()
    opt, _ = ap.parse_known_args()
    if opt.per_image and not opt.per_image.endswith(".npy"):
        ap.error("--per_image takes a .npy path")
    source = None if opt.tokens else E.image_source(opt, ap)
    labels = None
    if opt.labels:
        try:
            labels = E.read_labels(opt.labels)
        except (OSError, ValueError) as e:
            ap.error(f"--labels: {e}")
    import numpy as np
    from dynamicvectorquantization_amd import runtime as rt
    rt.set_compute_dtype(opt.dtype)
    model, size = E.load_stage2_model(opt.yaml_path, opt.model_path, "cuda", use_ema=opt.use_ema)
    if opt.tokens:
        from dynamicvectorquantization_amd import tokens as T
        ds = T.TokenShardDataset(opt.tokens)
        ds.check_model(model)
        if not 0 <= opt.view < ds.n_views:
            ap.error(f"--view {opt.view}: {opt.tokens} stores {ds.n_views} views per image")
        loader = T.TokenBatchLoader(ds, opt.batch_size, "cuda", model.permuter, shuffle=False, drop_last=False, view=opt.view)
        batches = token_batches(loader, opt.limit, model.cond_stage_key if model.cond_stage_key != model.first_stage_key else None, ap)
    else:
        batches = E.image_batches(opt.batch_size, size, "cuda", source, opt.synthetic, opt.limit, device_decode=opt.device_jpeg, device_png=opt.device_png)
    if not opt.tokens and model.cond_stage_key != model.first_stage_key:
        if labels is None:
            ap.error(f"{opt.yaml_path} is class-conditional: give --labels")
        n_classes = getattr(model, "n_classes", None)
        if n_classes is not None and labels.size and (labels.min() < 0 or labels.max() >= n_classes):
            ap.error(f"--labels: values outside [0, {n_classes})")
        batches = labelled_batches(batches, labels, model.cond_stage_key)
    s = E.evaluate_likelihood(model, batches, per_image=bool(opt.per_image))
    if opt.per_image:
        np.save(opt.per_image, s.pop("per_image"))
    line = json.dumps(s)
    if opt.json:
        with open(opt.json, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
