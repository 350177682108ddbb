#!/usr/bin/env python3
"""What training stage 2 from a token set saves (docs/design/16-token-shards.md).

configs/stage2/uncond_imagenet_p6c18.yml, random weights, bf16, batch 30, half-flat synthetic images (bench_extra.py --workload stage2);
HIP events after a warm-up, alternating rounds, minimum over the rounds (docs/design/07-measurement.md):
  (a) ms per training step from image batches already on the device (frozen DQ-VAE -> permuter with its host read -> StackGPT) against
      ms per step from a TokenBatchLoader over a token set made from the same images, same Trainer, same process
  (b) us per call of dvq_tokens_unpack and of dvq_permute_dual on the batch's product grid, and the host time of one
      DualGrainSeperatePermuter.forward (launch + the .tolist() wait) with the stream otherwise idle
  (c) the tokeniser's images/s
Writes the table to --out (and prints it).

    python tools/token_timing.py --out profiles/token_timing.txt
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--batches", type=int, default=4, help="distinct batches (the token set holds batch * batches images)")
    ap.add_argument("--steps", type=int, default=8, help="training steps per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200, help="calls per kernel timing")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import numpy as np
    import torch

    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd import tokens as T
    from dynamicvectorquantization_amd.kernels import lib
    from dynamicvectorquantization_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    rt.set_compute_dtype(opt.dtype)
    yml = os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml")
    bs = opt.batch
    model, size = E.load_stage2_model(yml, "", dev)
    fs, perm = model.first_stage_model, model.permuter
    hw1, hw2 = model.hw1, model.hw2
    images = [torch.from_numpy(synth.half_flat_images(bs, size, seed=300 + i)).to(dev) for i in range(opt.batches)]

    tmp = tempfile.mkdtemp(prefix="token_timing_")
    try:
        def tokenise(path):
            w = T.TokenShardWriter(path, hw1, hw2, fs.quantize.codebook.n_embed, ["center"], compute_dtype=E.dtype_name(),
                                   fingerprint=T.first_stage_fingerprint(fs), dataset={"synthetic": bs * opt.batches})
            st = T.tokenize_batches(fs, [([x], np.full(bs, -1), np.arange(i * bs, (i + 1) * bs)) for i, x in enumerate(images)], w)
            w.close()
            return st
        tokenise(os.path.join(tmp, "warm"))                                # first encode of this shape: packing, workspace
        tok_stats = [tokenise(os.path.join(tmp, f"set{r}")) for r in range(opt.rounds)]
        ds = T.TokenShardDataset(os.path.join(tmp, "set0"), verify=True)
        ds.check_model(model)
        loader = T.TokenBatchLoader(ds, bs, dev, perm, shuffle=False)

        def token_feed():
            while True:
                for b in loader:
                    yield b
        tfeed = token_feed()

        model.learning_rate, model.min_learning_rate = 1e-5, 0.0
        model.steps_per_epoch, model.training_steps = 1000, 100000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=False)
        step = [0]

        def image_steps(n):
            for _ in range(n):
                tr.train_step({"image": images[step[0] % opt.batches]}, step[0])
                step[0] += 1

        def token_steps(n):
            for _ in range(n):
                tr.train_step(next(tfeed), step[0])
                step[0] += 1

        def timed(fn, n):
            """(ms per call by HIP events, ms per call on the host clock up to the synchronise)"""
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            fn(n)
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / n, (time.perf_counter() - t0) * 1e3 / n

        for _ in range(2):
            image_steps(3)
            token_steps(3)
        img, tok = [], []
        for _ in range(opt.rounds):
            img.append(timed(image_steps, opt.steps))
            tok.append(timed(token_steps, opt.steps))

        # ---- (b) the two kernels on one batch of the product grid, and the permuter's host wait
        model.eval()
        with torch.no_grad():
            enc = fs.encode(images[0])
        idx, grain = enc[2][2].contiguous().long(), enc[3].contiguous().long()
        codes, bits, n_fine, _ = K.tokens_pack(idx, grain, fs.quantize.codebook.n_embed)
        n = n_fine.cpu().numpy()
        lc, lf = T.row_lengths(n, hw1, hw2)
        ncell, npix = hw1 * hw1, (hw1 * hw2) ** 2
        c6 = (perm.content_pad_code, perm.content_eos_code, perm.coarse_position_pad_code, perm.coarse_position_eos_code,
              perm.fine_position_pad_code, perm.fine_position_eos_code)
        order = 0 if perm.fine_position_order == "region-first" else 1
        ou = [torch.empty(bs, l, dtype=torch.long, device=dev) for l in (lc, lc, lf, lf)]
        op = [torch.empty(bs, l + 1, dtype=torch.long, device=dev) for l in (ncell, ncell, npix, npix)]
        counts = torch.empty(bs, 2, dtype=torch.int32, device=dev)
        p, s = K._p, K._s

        def unpack(reps):
            for _ in range(reps):
                lib().dvq_tokens_unpack(p(codes), p(bits), bs, hw1, hw2, order, *c6, lc, lf, p(ou[0]), p(ou[1]), p(ou[2]), p(ou[3]), s())

        def permute(reps):
            for _ in range(reps):
                lib().dvq_permute_dual(p(idx), p(grain), bs, hw1, hw2, order, *c6, p(op[0]), p(op[1]), p(op[2]), p(op[3]), p(counts), s())

        unpack(5)
        permute(5)
        t_unpack, t_permute = [], []
        for _ in range(opt.rounds):
            t_unpack.append(timed(unpack, opt.reps)[0] * 1e3)
            t_permute.append(timed(permute, opt.reps)[0] * 1e3)
        want = perm(indices=idx, grain_indices=grain)
        got = K.tokens_unpack(codes, bits, hw1, hw2, perm.fine_position_order, c6, lc, lf, n)
        same = all(torch.equal(want[k], got[k]) for k in T.STREAM_KEYS)

        def host_ms(fn, reps=20):
            out = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                out.append((time.perf_counter() - t0) * 1e3)
            return min(out), float(np.median(out))
        h_perm = host_ms(lambda: perm(indices=idx, grain_indices=grain))
        h_unpack = host_ms(lambda: K.tokens_unpack(codes, bits, hw1, hw2, perm.fine_position_order, c6, lc, lf, n))
        rec = ds.gather(np.arange(bs), np.zeros(bs, dtype=np.int64))
        h_len = host_ms(lambda: T.batch_lengths(rec["grain"], rec["n_fine_cells"], hw1, hw2))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    fmt = lambda v, u="ms": "  ".join(f"{x:8.3f}" for x in v) + f"   min {min(v):8.3f} {u}"
    ie, te = [a for a, _ in img], [a for a, _ in tok]
    ih, th = [b for _, b in img], [b for _, b in tok]
    ips = [s_["images_per_s"] for s_ in tok_stats]
    lines = [
        f"stage-2 training from a token set, uncond_imagenet_p6c18.yml, random weights, {opt.dtype}, batch {bs} x {size} x {size} half-flat, "
        f"{torch.cuda.get_device_name(0)} (tools/token_timing.py; HIP events, after warm-up, {opt.rounds} alternating rounds)",
        "",
        f"(a) ms per training step, {opt.steps} eager steps per window (grid {hw1} x {hw1}, hw2 {hw2}; Lc {lc}, Lf {lf}):",
        f"  image batches on the device, HIP events   {fmt(ie)}",
        f"  TokenBatchLoader batches,    HIP events   {fmt(te)}",
        f"  image batches on the device, host clock   {fmt(ih)}",
        f"  TokenBatchLoader batches,    host clock   {fmt(th)}",
        f"  token / image (min over rounds): HIP events {min(te) / min(ie):.3f}x, host clock {min(th) / min(ih):.3f}x;  saved per step "
        f"{min(ie) - min(te):.3f} ms (events) {min(ih) - min(th):.3f} ms (host)",
        "",
        f"(b) one batch of {bs} on the product grid, {opt.reps} calls per window (streams bit-equal: {same}):",
        f"  dvq_tokens_unpack (rows {lc} / {lf})       {fmt(t_unpack, 'us')}",
        f"  dvq_permute_dual  (rows {ncell + 1} / {npix + 1})     {fmt(t_permute, 'us')}",
        f"  host clock, stream idle: DualGrainSeperatePermuter.forward (launch + .tolist() wait + 4 slices)   min {h_perm[0]:.3f} ms  "
        f"median {h_perm[1]:.3f} ms",
        f"  host clock, stream idle: kernels.tokens_unpack (checks + allocations + launch, no wait)         min {h_unpack[0]:.3f} ms  "
        f"median {h_unpack[1]:.3f} ms",
        f"  host clock: popcount + row lengths of the batch's bitmaps (tokens.batch_lengths)                min {h_len[0]:.3f} ms  "
        f"median {h_len[1]:.3f} ms",
        "",
        f"(c) tokeniser (encode + dvq_tokens_pack + one host copy per batch + writer), {bs * opt.batches} images per run:",
        f"  images/s                                  {fmt(ips, 'img/s')}   (max {max(ips):.1f})",
        f"  tokens per image mean {tok_stats[0]['tokens_per_image']['mean']:.1f}, fine ratio {tok_stats[0]['fine_ratio']:.3f}, "
        f"record {ds.dtype.itemsize} bytes",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
