#!/usr/bin/env python3
"""Class-conditional sampling with a DQ-Transformer (ClassDualformer), optionally with classifier-free guidance
(docs/design/14-guidance.md).  The flags and output layout of sample_dynamic_uncond.py (its helpers are imported, not copied), plus:

    --classes     0-999, or a comma list (default: every class of the model)
    --per_class   samples per class (default 50: the ImageNet FID-50k protocol)
    --cfg_scale   guidance scale s (default 1.0 = plain conditional batches, no null half: runs on tables without a null row)
    --npz         also write samples_<N>x<H>x<W>x3.npz: arr_0 uint8 NHWC images, arr_1 int64 labels, in class order

The labels are the classes in the given order, each repeated --per_class times, cut into batches of --batch_size.  A guided batch
is 2 x batch_size rows (labels, then null labels); up to 64 rows it stays on the persistent decode kernel.

    python scripts/sample_val/sample_dynamic_class.py --yaml_path configs/stage2/class_imagenet_p6c18_cfg.yml \\
        --model_path last.ckpt --cfg_scale 2 --top_k 300 --top_k_pos 1024 --npz
"""
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import sample_dynamic_uncond as uncond  # noqa: E402

DECODE_STACK_ROWS = 64          # dvq_decode_stack's batch limit: larger batches fall back to per-kernel token steps


def parse_classes(spec, n_classes):
    """'' -> every class; 'a-b' -> a .. b inclusive; 'a,b,c' -> that list (order kept; ranges may appear in the list)"""
    if spec is None or spec.strip() == "":
        return list(range(n_classes))
    out = []
    for part in spec.split(","):
        part = part.strip()
        if not part:
            continue
        if "-" in part:
            lo, hi = (int(x) for x in part.split("-", 1))
            if hi < lo:
                raise ValueError(f"--classes: empty range {part}")
            out.extend(range(lo, hi + 1))
        else:
            out.append(int(part))
    if not out:
        raise ValueError(f"--classes: no class in {spec!r}")
    bad = [c for c in out if not 0 <= c < n_classes]
    if bad:
        raise ValueError(f"--classes: {bad[:5]} outside [0, {n_classes})")
    return out


def to_uint8_nhwc(img):
    """[N,3,H,W] float in [0,1] -> uint8 [N,H,W,3] (round to nearest)"""
    import numpy as np
    return (np.asarray(img, dtype=np.float32).transpose(0, 2, 3, 1) * 255.0 + 0.5).clip(0, 255).astype(np.uint8)


def write_npz(directory, images_u8, labels):
    """samples_<N>x<H>x<W>x3.npz with arr_0 = uint8 NHWC images and arr_1 = int64 labels (the layout ImageNet FID evaluators read)"""
    import numpy as np
    images_u8 = np.asarray(images_u8)
    labels = np.asarray(labels, dtype=np.int64)
    assert images_u8.dtype == np.uint8 and images_u8.ndim == 4 and images_u8.shape[3] == 3, images_u8.shape
    assert labels.shape == (images_u8.shape[0],), (labels.shape, images_u8.shape)
    n, h, w, _ = images_u8.shape
    path = os.path.join(directory, f"samples_{n}x{h}x{w}x3.npz")
    np.savez(path, arr_0=images_u8, arr_1=labels)
    return path


def get_parser():
    parser = uncond.get_parser()
    parser.set_defaults(batch_size=32)
    parser.add_argument("--classes", type=str, default="")
    parser.add_argument("--per_class", type=int, default=50)
    parser.add_argument("--cfg_scale", type=float, default=1.0)
    parser.add_argument("--npz", action="store_true", default=False)
    return parser


def main():
    opt = get_parser().parse_args()
    import time

    import numpy as np
    import torch
    from dynamicvectorquantization_amd import config as cfg, runtime as rt
    rt.set_compute_dtype(opt.dtype)
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
    model = cfg.instantiate_from_config(cfg.load_yaml(opt.yaml_path).model)
    if not hasattr(model, "guided_conditioning"):
        raise SystemExit(f"{opt.yaml_path}: not a class-conditional model")
    if opt.model_path:
        from dynamicvectorquantization_amd.evaluate import load_checkpoint_state_dict
        model.load_state_dict(load_checkpoint_state_dict(opt.model_path, opt.use_ema))
    model = model.eval().cuda()
    classes = parse_classes(opt.classes, model.n_classes)
    labels = np.repeat(np.asarray(classes, dtype=np.int64), opt.per_class)
    n_total = int(labels.shape[0])
    guided = opt.cfg_scale != 1.0

    now = datetime.datetime.utcnow().strftime("%m-%dT%H-%M-%S")
    base = opt.out_dir or (opt.model_path.replace(".ckpt", "") if opt.model_path else "samples") + "_{}_Num-{}/".format(now, n_total)
    tag = "TopK-{}-{}_TopP-{}-{}_Temp-{}_CFG-{}".format(opt.top_k, opt.top_k_pos, opt.top_p, opt.top_p_pos, opt.temperature,
                                                         opt.cfg_scale)
    if opt.sample_with_fixed_pos:
        tag = "fixed_" + tag
    dir_img, dir_pkl, dir_npz = (os.path.join(base, tag + s) for s in ("_image", "_pickle", "_npz"))
    if opt.save_image:
        os.makedirs(dir_img, exist_ok=True)
    os.makedirs(dir_pkl, exist_ok=True)
    if opt.npz:
        os.makedirs(dir_npz, exist_ok=True)
    if guided and 2 * opt.batch_size > DECODE_STACK_ROWS:
        print(f"note: a guided batch is {2 * opt.batch_size} rows (> {DECODE_STACK_ROWS}): token steps leave the persistent decode "
              f"kernel; --batch_size {DECODE_STACK_ROWS // 2} keeps it")

    total_batch = (n_total + opt.batch_size - 1) // opt.batch_size
    starts = [i * opt.batch_size for i in range(total_batch)]
    sizes = [min(opt.batch_size, n_total - s) for s in starts]
    kw = dict(temperature=opt.temperature, sample=True, top_k=opt.top_k, top_p=opt.top_p, top_k_pos=opt.top_k_pos, top_p_pos=opt.top_p_pos,
              process=False, fix_fine_position=opt.sample_with_fixed_pos, cfg_scale=opt.cfg_scale if guided else None)
    group = max(1, opt.streams) * 4
    all_u8 = []
    steps, t0 = 0, time.perf_counter()
    with torch.no_grad():
        for g0 in range(0, total_batch, group):
            idxs = list(range(g0, min(total_batch, g0 + group)))
            conds = {}
            for i in idxs:
                lab = torch.from_numpy(labels[starts[i]:starts[i] + sizes[i]]).cuda()
                conds[i] = model.guided_conditioning(lab) if guided else model.encode_to_c(lab)
            # full batches through the concurrent lanes; a ragged last batch (another cache geometry) on its own
            full = [i for i in idxs if sizes[i] == opt.batch_size]
            outs = dict(zip(full, model.sample_many([conds[i] for i in full], n_streams=opt.streams, **kw))) if full else {}
            for i in idxs:
                if i not in outs:
                    outs[i] = model.sample_from_scratch(*conds[i], **kw)
            for i in idxs:
                seqs = outs[i]
                steps += sizes[i] * int(seqs[0].shape[1] + seqs[1].shape[1])
                img = torch.clamp(model.decode_to_img(*seqs).float() * 0.5 + 0.5, 0, 1).cpu().numpy()
                if opt.save_image:
                    uncond.save_image_grid(img, os.path.join(dir_img, "batch_{}.png".format(i)))
                uncond.save_pickle(os.path.join(dir_pkl, "samples_({}_{}).pkl".format(i, total_batch)), img)
                if opt.npz:
                    all_u8.append(to_uint8_nhwc(img))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if opt.npz:
        print("wrote", write_npz(dir_npz, np.concatenate(all_u8, axis=0), labels))
    print("sampled {} images of {} classes (cfg_scale {}), {} token steps in {:.2f} s ({:.2f} images/s, {:.0f} token-steps/s) -> {}".format(
        n_total, len(classes), opt.cfg_scale, steps, dt, n_total / dt, steps / dt, dir_pkl))


if __name__ == "__main__":
    main()
