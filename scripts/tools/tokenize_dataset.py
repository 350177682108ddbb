#!/usr/bin/env python3
"""Tokenise a dataset with a frozen DQ-VAE into a token set (docs/design/16-token-shards.md): every image is encoded once per stored
view, the code map and the grain map are packed on the device (dvq_tokens_pack) and written as fixed-size records.  Stage 2 then trains
(`train.py --token_data DIR`) and scores (`eval_likelihood.py --tokens DIR`) without the first stage and without decoding images.
Prints ONE JSON line: images, views, records, tokens per image, fine ratio, seconds, images/s.

    python scripts/tools/tokenize_dataset.py --yaml_path configs/stage2/uncond_imagenet_p6c18.yml --model_path stage1.ckpt \\
        --split train --views random:4 --out tokens/train --batch_size 64

--views center | center,flip | random:N.  `flip` is the centre crop mirrored BEFORE encoding (a mirrored code map is not the code map
of the mirrored image); random:N is N draws of the training transform (RandomCrop + RandomHorizontalFlip) per image, seeded by
(--seed, image index, view) and therefore independent of --batch_size and --part.  --part I/N tokenises the I-th of N contiguous slices
(files tokens-pIIII-*.npy); --finalize checks that every part is there and writes meta.json.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from dynamicvectorquantization_amd import evaluate as E  # noqa: E402
from dynamicvectorquantization_amd import tokens as T  # noqa: E402
from dynamicvectorquantization_amd.quantize import codebook_of  # noqa: E402


def get_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    E.add_eval_args(ap)
    ap.add_argument("--split", type=str, default="", choices=["", "train", "validation"], help="the YAML's own data: section")
    ap.add_argument("--out", type=str, required=True)
    ap.add_argument("--views", type=str, default="center")
    ap.add_argument("--shard_size", type=int, default=65536, help="records per file")
    ap.add_argument("--part", type=str, default="", help="I/N: tokenise the I-th of N contiguous slices of the dataset")
    ap.add_argument("--finalize", action="store_true", help="write meta.json from the parts already in --out, tokenise nothing")
    ap.add_argument("--seed", type=int, default=2021)
    ap.add_argument("--num_workers", type=int, default=8)
    return ap


def parse_views(spec, ap):
    if spec.startswith("random:"):
        try:
            n = int(spec[7:])
        except ValueError:
            n = 0
        if not 0 < n <= 255:
            ap.error(f"--views {spec}: random:N with N in 1 .. 255")
        return [f"random:{i}" for i in range(n)]
    views = spec.split(",")
    if views not in (["center"], ["center", "flip"]):
        ap.error(f"--views {spec}: center | center,flip | random:N")
    return views


def load_first_stage(yaml_path, model_path, device, use_ema=False):
    """the DQ-VAE of a stage-1 YAML, or of a stage-2 YAML's first_stage_config (a stage-2 checkpoint's first_stage_model.* entries
    load too).  -> (model in eval mode, image size)"""
    import torch

    from dynamicvectorquantization_amd import config as cfg
    conf = cfg.load_yaml(yaml_path)
    mconf = conf.model
    if "first_stage_config" in mconf.params:
        mconf = mconf.params.first_stage_config
    torch.manual_seed(0)
    model = cfg.instantiate_from_config(mconf)
    if model_path:
        sd = E.load_checkpoint_state_dict(model_path, use_ema)
        inner = {k[len("first_stage_model."):]: v for k, v in sd.items() if k.startswith("first_stage_model.")}
        model.load_state_dict(inner or sd)
    size = mconf.params.get("image_size") or mconf.params.encoderconfig.params.resolution
    return model.eval().to(device), int(size)


def tensor_view_batches(batches, views, lo, hi):
    """already transformed image tensors (--synthetic, .npy): the image as it is, and its mirror image"""
    import numpy as np
    import torch
    i = 0
    for x in batches:
        b = int(x.shape[0])
        a, z = max(lo, i), min(hi, i + b)
        if a < z:
            x = x[a - i:z - i].contiguous()
            yield [x if v == "center" else torch.flip(x, dims=[3]).contiguous() for v in views], np.full(z - a, -1), np.arange(a, z)
        i += b


def decoded_view_batches(ds, views, lo, hi, batch_size, size, device, seed, workers, device_decode=False, device_png=False):
    """decoded images (a folder, the YAML's dataset): data.plan_batch per view with the view's crops / flips, the transforms on the GPU.
    device_decode: JPEG files are decoded on the GPU too, once per batch (data.decode_batch_gpu); every view reads that buffer.
    device_png: the same for PNG files (docs/design/29-device-png.md)"""
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    from dynamicvectorquantization_amd import data
    with ThreadPoolExecutor(max(1, workers)) as pool:
        for i in range(lo, hi, batch_size):
            idx = list(range(i, min(hi, i + batch_size)))
            ex = list(pool.map((lambda j: ds.example(j, device_decode, device_png)) if device_decode or device_png else ds.__getitem__, idx))
            dec = None
            if any("jpeg" in e or "png" in e for e in ex):
                dec = data.decode_batch_gpu([data.example_record(e) for e in ex], device)
            sizes = dec["sizes"] if dec else [(int(e["image_u8"].shape[1]), int(e["image_u8"].shape[0])) for e in ex]
            out = []
            for v, name in enumerate(views):
                crops = flips = None
                if name == "flip":
                    flips = [True] * len(ex)
                elif name.startswith("random:"):
                    crops, flips = [], []
                    for j, (w, h) in zip(idx, sizes):
                        rng = np.random.default_rng([seed, j, v])
                        nw, nh = data.resized_size(w, h, size)
                        cy, cx = int(rng.integers(0, nh - size + 1)), int(rng.integers(0, nw - size + 1))      # RandomCrop.get_params: i, j
                        crops.append((cx, cy))
                        flips.append(bool(rng.random() < 0.5))
                if dec:
                    plan = data.plan_batch_sizes(sizes, size, crops=crops, flips=flips, src_offs=dec["offs"])
                    out.append(data.transform_batch_device(plan, dec["rgb"], device))
                else:
                    out.append(data.transform_batch_gpu(data.plan_batch([e["image_u8"] for e in ex], size, crops=crops, flips=flips), device))
            labels = np.array([int(e.get("class_label", -1)) for e in ex], dtype=np.int64)
            yield out, labels, np.array(idx)


def main():
    ap = get_parser()
    opt, _ = ap.parse_known_args()
    if opt.finalize:
        meta = T.finalize_parts(opt.out)
        print(json.dumps({"finalized": opt.out, "parts": meta["parts"], "records": meta["records"], "files": len(meta["files"])}))
        return
    views = parse_views(opt.views, ap)
    part = None
    if opt.part:
        try:
            part = tuple(int(v) for v in opt.part.split("/"))
            assert len(part) == 2 and 0 <= part[0] < part[1]
        except (ValueError, AssertionError):
            ap.error(f"--part {opt.part}: I/N with 0 <= I < N")
    source = None if opt.split else E.image_source(opt, ap)
    import torch

    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import runtime as rt
    rt.set_compute_dtype(opt.dtype)
    dev = torch.device("cuda")
    model, size = load_first_stage(opt.yaml_path, opt.model_path, dev, use_ema=opt.use_ema)
    hw1, hw2 = T.first_stage_grid(model, size, dev)

    ds = None
    if opt.split:
        ds = cfg.instantiate_from_config(cfg.load_yaml(opt.yaml_path).data.params[opt.split])
        n, described = len(ds), {"yaml_path": opt.yaml_path, "split": opt.split}
    elif source is None:
        n, described = opt.synthetic, {"synthetic": opt.synthetic, "seed": 2021}
    elif source.endswith(".npy"):
        import numpy as np
        n, described = int(np.load(source, mmap_mode="r").shape[0]), {"images": source}
    else:
        ds = E.folder_dataset(source, None)
        n, described = len(ds), {"images": source}
    if opt.limit:
        n = min(n, opt.limit)
    described.update(n_images=n, image_size=size, seed=opt.seed)
    lo, hi = (0, n) if part is None else (n * part[0] // part[1], n * (part[0] + 1) // part[1])
    if ds is None:
        if any(v.startswith("random:") for v in views):
            ap.error("--views random:N draws crops of decoded images: give a folder (--images DIR) or --split")
        batches = tensor_view_batches(E.image_batches(opt.batch_size, size, dev, source, opt.synthetic, n, device_decode=opt.device_jpeg, device_png=opt.device_png), views, lo, hi)
    else:
        batches = decoded_view_batches(ds, views, lo, hi, opt.batch_size, size, dev, opt.seed, opt.num_workers, opt.device_jpeg, opt.device_png)
    writer = T.TokenShardWriter(opt.out, hw1, hw2, codebook_of(model.quantize)[1], views, shard_size=opt.shard_size,
                                compute_dtype=E.dtype_name(), fingerprint=T.first_stage_fingerprint(model), dataset=described, part=part)
    stats = T.tokenize_batches(model, batches, writer)
    writer.close()
    stats.update(out=opt.out, part=list(part) if part else None, dtype=E.dtype_name(), hw1=hw1, hw2=hw2)
    print(json.dumps(stats))


if __name__ == "__main__":
    main()
