#!/usr/bin/env python3
"""Lossless token codec (docs/design/27-token-codec.md): rANS-code images -- or the stored codes of a token set -- with a DQ-Transformer
as the entropy model, and decode such a file back to code indices and grain maps.

    python scripts/tools/compress_images.py compress --yaml_path configs/stage2/uncond_imagenet_p6c18.yml --model_path last.ckpt \\
        --images photos/ --group 8 --out photos.dqtc --verify
    python scripts/tools/compress_images.py decompress --yaml_path configs/stage2/uncond_imagenet_p6c18.yml --model_path last.ckpt \\
        --input photos.dqtc --out codes.npz [--images_out images.npy]

compress prints ONE JSON line: images, bytes per image (payload and whole file), ideal bits per image by stream and the coder's
overhead.  --tokens DIR codes a token set (scripts/tools/tokenize_dataset.py) instead of images (--view K).  A class-conditional model
needs --labels for images and takes the stored labels of a token set.  --verify decodes what was just written and compares the tokens.
A file decodes only under the checkpoint, the compute dtype and the build that wrote it; decompress --force tries anyway.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from dynamicvectorquantization_amd import evaluate as E  # noqa: E402


def get_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    c = sub.add_parser("compress")
    E.add_eval_args(c)
    c.add_argument("--out", type=str, required=True, help="the container file to write")
    c.add_argument("--group", type=int, default=8, help="images coded together (and decoded together)")
    c.add_argument("--labels", type=str, default="", help="class labels of a class-conditional model: .npy or text file, image order")
    c.add_argument("--tokens", type=str, default="", help="code this token set instead of images")
    c.add_argument("--view", type=int, default=0, help="--tokens: the stored view of every image to code")
    c.add_argument("--verify", action="store_true", help="decode the file just written and compare the tokens")
    d = sub.add_parser("decompress")
    d.add_argument("--yaml_path", type=str, required=True)
    d.add_argument("--model_path", type=str, default="")
    d.add_argument("--use_ema", action="store_true")
    d.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp32x3"])
    d.add_argument("--input", type=str, required=True, help="a container written by `compress`")
    d.add_argument("--out", type=str, required=True, help=".npz with indices [N, fine_hw, fine_hw] and grain_indices [N, hw, hw]")
    d.add_argument("--images_out", type=str, default="", help="also decode to images: [N, 3, H, W] fp32 .npy")
    d.add_argument("--force", action="store_true", help="decode under another checkpoint / compute dtype than the file names")
    return ap


def gather_tokens(opt, ap, model, size):
    """(tokens dict of all images, labels tensor or None)"""
    import torch
    from dynamicvectorquantization_amd import codec
    label_key = model.cond_stage_key if model.cond_stage_key != model.first_stage_key else None
    zs, labs = [], []
    if opt.tokens:
        from dynamicvectorquantization_amd import tokens as T
        ds = T.TokenShardDataset(opt.tokens)
        ds.check_model(model)
        if not 0 <= opt.view < ds.n_views:
            ap.error(f"--view {opt.view}: {opt.tokens} stores {ds.n_views} views per image")
        n = 0
        for b in T.TokenBatchLoader(ds, opt.batch_size, "cuda", model.permuter, shuffle=False, drop_last=False, view=opt.view):
            if label_key is not None and label_key not in b:
                ap.error("the model is class-conditional and this token set stores no labels")
            k = len(b["n_tokens"])
            if opt.limit:
                k = min(k, opt.limit - n)
                if k <= 0:
                    break
            zs.append({key: v[:k] for key, v in b["tokens"].items()})
            if label_key is not None:
                labs.append(b[label_key][:k].reshape(-1))
            n += k
    else:
        labels = None
        if label_key is not None:
            if not opt.labels:
                ap.error(f"{opt.yaml_path} is class-conditional: give --labels")
            labels = torch.from_numpy(E.read_labels(opt.labels))
        n = 0
        for x in E.image_batches(opt.group * max(1, opt.batch_size // opt.group), size, "cuda", E.image_source(opt, ap), opt.synthetic,
                                 opt.limit, device_decode=opt.device_jpeg, device_png=opt.device_png):
            for g0 in range(0, x.shape[0], opt.group):          # tokenised group by group, as Dualformer.compress does
                zs.append(model.encode_to_z(x[g0:g0 + opt.group])[1])
            n += int(x.shape[0])
        if labels is not None:
            if labels.numel() < n:
                ap.error(f"--labels holds {labels.numel()} labels, the images need {n}")
            labs.append(labels[:n].to("cuda"))
    if not zs:
        ap.error("no images")
    return codec.cat_tokens(model, zs), (torch.cat(labs) if labs else None)


def main():
    ap = get_parser()
    opt = ap.parse_args()
    import numpy as np
    import torch

    from dynamicvectorquantization_amd import codec
    from dynamicvectorquantization_amd import runtime as rt
    rt.set_compute_dtype(opt.dtype)
    model, size = E.load_stage2_model(opt.yaml_path, opt.model_path, "cuda", use_ema=opt.use_ema)
    with torch.no_grad():
        if opt.command == "decompress":
            with open(opt.input, "rb") as f:
                blob = f.read()
            try:
                decoded = codec.decompress_tokens(model, blob, force=opt.force)       # one pass of the token loop for both outputs
                idx, grain = codec.codes_of(model, decoded)
                np.savez(opt.out, indices=idx.cpu().numpy(), grain_indices=grain.cpu().numpy())
                if opt.images_out:
                    np.save(opt.images_out, codec.images_of(model, decoded).float().cpu().numpy())
            except codec.CodecError as e:
                raise SystemExit(f"{opt.input}: {e}")
            print(json.dumps({"images": int(idx.shape[0]), "bytes": len(blob)}))
            return
        tokens, labels = gather_tokens(opt, ap, model, size)
        blob, bits = model.compress_tokens(tokens, labels, batch_group=opt.group, return_bits=True)
        with open(opt.out, "wb") as f:
            f.write(blob)
        n = int(bits.shape[0])
        payload = codec.payload_bits(blob)
        ideal = bits.cpu().numpy()
        s = {"images": n, "group": opt.group, "file_bytes": len(blob), "file_bytes_per_image": len(blob) / n,
             "payload_bytes_per_image": float(payload.mean()) / 8,
             "ideal_bits_per_image": {"coarse_position": float(ideal[:, 0].mean()), "coarse_content": float(ideal[:, 1].mean()),
                                      "fine_content": float(ideal[:, 2].mean()), "total": float(ideal.sum(axis=1).mean())},
             "overhead_bits_per_image": float((payload - ideal.sum(axis=1)).mean())}
        if opt.verify:
            with open(opt.out, "rb") as f:
                back = f.read()
            idx, grain = model.decompress(back)
            want = model.permuter.forward_back(tokens["coarse_content"], tokens["fine_content"], tokens["coarse_position"],
                                               tokens["fine_position"])
            want_grain = 1 - model._coarse_cells_drawn(torch.nn.functional.pad(tokens["coarse_position"], (1, 0), value=0))
            s["verified"] = bool(torch.equal(idx, want) and torch.equal(grain, want_grain))
            if not s["verified"]:
                print(json.dumps(s))
                raise SystemExit("verification FAILED: the decoded tokens differ from the coded ones")
        print(json.dumps(s))


if __name__ == "__main__":
    main()
