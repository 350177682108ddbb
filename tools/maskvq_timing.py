#!/usr/bin/env python3
"""What the gradient-trained codebook costs (docs/design/17-trained-codebook.md).  One GPU visit, HIP events after a warm-up, alternating
rounds, minimum over the rounds (docs/design/07-measurement.md):
  (a) dvq_vq_sample_argmax at N 65 536, K 1024, D 256: bf16 rows with Gumbel noise against the exact search (dvq_vq_argmin) on fp32 rows
      at the same shape in the same run -- the three-product case, the nearest thing the EMA path has -- and the split of the new kernel:
      its MFMA loop alone (temp 0, no noise) against the loop with the noise arithmetic, for bf16 and fp32 rows
  (b) dvq_vq_codebook_grad against dvq_vq_ema_stats at the same shape and assignment: skewed (90 % of the rows on one code), the argmin
      against an untrained codebook, and a uniform one
  (c) one headline-shaped training step (bs 64, bf16, Trainer with its recorded step) of the trained-codebook YAML against the EMA
      YAML, both models alive in one process, alternating windows (reported only)
Writes the table to --out (and prints it).

    python tools/maskvq_timing.py --out profiles/maskvq_timing.txt
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50, help="calls per kernel timing window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed window")
    ap.add_argument("--no-step", action="store_true", help="skip (c)")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import numpy as np
    import torch

    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import synth
    dev = torch.device("cuda:0")
    n, k, d = opt.n, opt.k, opt.d

    def timed(fn, reps):
        """ms per call by HIP events"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    def rounds(fns, reps):
        """{name: [ms per round]}: warm every candidate, then alternate them round by round"""
        for f in fns.values():
            for _ in range(5):
                f()
        out = {name: [] for name in fns}
        for _ in range(opt.rounds):
            for name, f in fns.items():
                out[name].append(timed(f, reps))
        return out

    fmt = lambda v, u="ms": "  ".join(f"{x:8.4f}" for x in v) + f"   min {min(v):8.4f} {u}"
    lines = [f"gradient-trained codebook (MaskVectorQuantize) kernels, {torch.cuda.get_device_name(0)} "
             f"(tools/maskvq_timing.py; HIP events, after warm-up, {opt.rounds} alternating rounds, {opt.reps} calls per window)", ""]

    # ---- (a) the search ---------------------------------------------------------------------------------------------------------------
    x32, cb = (torch.from_numpy(a).to(dev) for a in synth.vq_inputs(n, d, k, "encoder", seed=1))
    cb = cb * float(k)                    # a codebook of the rows' own scale: the score gaps an early training step sees
    xb = x32.to(torch.bfloat16)
    prep_exact = K.vq_prepare(cb)
    prep = K.vq_trained_prepare(cb, False)
    prep_cos = K.vq_trained_prepare(cb, True)
    state = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    temp = 20.0
    res = rounds({
        "exact fp32": lambda: K.vq_argmin(x32, cb, prep_exact),
        "exact bf16": lambda: K.vq_argmin(xb, cb, prep_exact),
        "new bf16 noise": lambda: K.vq_sample_argmax(xb, prep, k, False, temp, state),
        "new bf16 plain": lambda: K.vq_sample_argmax(xb, prep, k, False, 0.0),
        "new fp32 noise": lambda: K.vq_sample_argmax(x32, prep, k, False, temp, state),
        "new fp32 plain": lambda: K.vq_sample_argmax(x32, prep, k, False, 0.0),
        "new bf16 cosine noise": lambda: K.vq_sample_argmax(xb, prep_cos, k, True, 0.05, state),
        "prepare": lambda: K.vq_trained_prepare(cb, False),
    }, opt.reps)
    yard = min(res["exact fp32"])
    lines += [f"(a) search, N {n}, K {k}, D {d} (rows ~ N(0, 12/D), codebook U(+-1) rows):",
              f"  dvq_vq_argmin, fp32 rows (exact, three products, pruned + fp64 re-rank): the yardstick   {fmt(res['exact fp32'])}",
              f"  dvq_vq_argmin, bf16 rows (exact, two products)                                          {fmt(res['exact bf16'])}",
              f"  dvq_vq_sample_argmax, bf16 rows, temp {temp} (Gumbel noise)                               {fmt(res['new bf16 noise'])}",
              f"  dvq_vq_sample_argmax, bf16 rows, temp 0 (its MFMA loop + running argmax alone)          {fmt(res['new bf16 plain'])}",
              f"  dvq_vq_sample_argmax, fp32 rows, temp {temp} (Gumbel noise)                               {fmt(res['new fp32 noise'])}",
              f"  dvq_vq_sample_argmax, fp32 rows, temp 0                                                 {fmt(res['new fp32 plain'])}",
              f"  dvq_vq_sample_argmax, bf16 rows, cosine, temp 0.05                                      {fmt(res['new bf16 cosine noise'])}",
              f"  dvq_vq_trained_prepare                                                                  {fmt(res['prepare'])}",
              f"  Gumbel search on bf16 rows / yardstick: {min(res['new bf16 noise']) / yard:.2f}x (allowance 2x); "
              f"noise share of the bf16 kernel: {1 - min(res['new bf16 plain']) / min(res['new bf16 noise']):.2f}", ""]

    # ---- (b) the codebook gradient ------------------------------------------------------------------------------------------------------
    cb0 = torch.from_numpy(synth.vq_inputs(n, d, k, "encoder", seed=1)[1]).to(dev)            # untrained: U(+-1/K)
    idx_untrained = K.vq_argmin(xb, cb0, K.vq_prepare(cb0))
    rs = np.random.RandomState(2)
    idx_skew = torch.from_numpy(np.where(rs.uniform(size=n) < 0.9, 7, rs.randint(0, k, size=n))).to(dev)       # 90 % on one code
    idx_uni = torch.from_numpy(np.random.RandomState(0).randint(0, k, size=n)).to(dev)
    mask = torch.from_numpy(np.where(np.random.RandomState(1).uniform(size=n) < 0.5, 0.25, 1.0).astype(np.float32)).to(dev)
    coef = torch.tensor([1e-3], dtype=torch.float32, device=dev)
    grad = torch.zeros(k, d, dtype=torch.float32, device=dev)
    stats = torch.empty(k, d + 1, dtype=torch.float32, device=dev)
    lines.append(f"(b) codebook gradient against the EMA statistics, N {n}, K {k}, D {d}, bf16 rows:")
    for name, idx in (("skewed: 90 % of the rows on one code", idx_skew), ("argmin against an untrained codebook", idx_untrained),
                      ("uniform assignment", idx_uni)):
        top = int(torch.bincount(idx, minlength=k).max())
        res = rounds({"ema": lambda: K.vq_ema_stats(xb, idx, k, out=stats),
                      "grad": lambda: K.vq_codebook_grad(xb, cb, idx, mask, coef, grad),
                      "grad nomask": lambda: K.vq_codebook_grad(xb, cb, idx, None, coef, grad)}, opt.reps)
        K.set_deterministic(True)
        try:
            det = rounds({"grad det": lambda: K.vq_codebook_grad(xb, cb, idx, mask, coef, grad)}, max(5, opt.reps // 5))
        finally:
            K.set_deterministic(False)
        lines += [f"  {name} (hottest code owns {top} rows, {int((torch.bincount(idx, minlength=k) > 0).sum())} codes used):",
                  f"    dvq_vq_ema_stats (zero fill + walk): the yardstick        {fmt(res['ema'])}",
                  f"    dvq_vq_codebook_grad, mask                                {fmt(res['grad'])}",
                  f"    dvq_vq_codebook_grad, no mask                             {fmt(res['grad nomask'])}",
                  f"    dvq_vq_codebook_grad, mask, deterministic mode            {fmt(det['grad det'])}",
                  f"    gradient / statistics: {min(res['grad']) / min(res['ema']):.2f}x (allowance 1.5x)"]
    lines.append("")

    # ---- (c) one training step of either YAML -------------------------------------------------------------------------------------------
    if not opt.no_step:
        from dynamicvectorquantization_amd import config
        from dynamicvectorquantization_amd import runtime as rt
        from dynamicvectorquantization_amd.trainer import Trainer
        yamls = {"EMA": "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml",
                 "trained": "configs/stage1/dqvae-entropy-dual-r05-trainedcb_imagenet.yml"}
        rt.set_compute_dtype("bf16")
        bs = opt.batch
        images = [torch.from_numpy(synth.half_flat_images(bs, 256, seed=500 + i)).to(dev) for i in range(2)]
        runs = {}
        for name, yml in yamls.items():
            torch.manual_seed(0)
            model = config.instantiate_from_config(config.stage1_config(yml, batch_size=bs).model).to(dev)
            model.learning_rate, model.min_learning_rate = 4.5e-6 * bs, 0.0
            model.steps_per_epoch, model.training_steps = 1000, 100000
            model.train()
            runs[name] = [model, Trainer(model, max_steps=100000), 0]

        def steps(run, cnt):
            for _ in range(cnt):
                run[1].train_step({"image": images[run[2] % 2]}, run[2])
                run[2] += 1

        for run in runs.values():
            steps(run, 8)                  # eager steps, the recording, first replays
        ms = {name: [] for name in runs}
        for _ in range(3):
            for name, run in runs.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                ev[0].record()
                steps(run, opt.steps)
                ev[1].record()
                torch.cuda.synchronize()
                ms[name].append(ev[0].elapsed_time(ev[1]) / opt.steps)
        lines += [f"(c) ms per training step, {yamls['trained']} against {yamls['EMA']}:",
                  f"    bs {bs}, bf16, 256 x 256 half-flat images, full objective, Trainer with its recorded step (replays: EMA "
                  f"{runs['EMA'][1].graph_replays}, trained {runs['trained'][1].graph_replays}), {opt.steps} steps per window:",
                  f"  EMA codebook (VectorQuantize2)            {fmt(ms['EMA'])}   {bs * 1e3 / min(ms['EMA']):.1f} img/s",
                  f"  trained codebook (MaskVectorQuantize)     {fmt(ms['trained'])}   {bs * 1e3 / min(ms['trained']):.1f} img/s",
                  f"  trained / EMA: {min(ms['trained']) / min(ms['EMA']):.4f}x"]

    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
