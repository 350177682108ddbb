#!/usr/bin/env python3
"""What the weight EMA costs (docs/design/20-weight-ema.md).

HIP events after a warm-up, alternating rounds in one process, minimum over the rounds (docs/design/07-measurement.md):
  (a) --part kernels: dvq_ema_update (12 bytes per element: reads e, p, writes e) and dvq_swap_f32 (16 bytes per element) alone on
      buffers of the flat sizes of the stage-2 optimizer and the two stage-1 optimizers, next to dvq_adamw_dev (28 bytes per element)
      measured in the same process on the same buffers
  (b) --part stage2 / stage1: ms per training step with the feature off against on, same Trainer, same process:
      stage 2 (configs/stage2/uncond_imagenet_p6c18.yml, bf16, batch 30, eager launches) and
      stage 1 (the benchmark's DQ-VAE, bf16, complete objective, the step recorded and replayed)
Each part is one process, so that a caller can give every part its own time limit; the table is appended to --out (and printed).

    for p in stage2 stage1 kernels; do python tools/ema_timing.py --part $p --out profiles/ema_timing.txt; done
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# flat sizes of the optimizers (docs/design/19-gradient-clipping.md, table (a)); parts stage2 / stage1 print their own for comparison
SIZES = {"stage 2 (StackGPT p6c18)": 308884480, "stage 1 generator": 47571331, "stage 1 discriminator": 2765633}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["stage2", "stage1", "kernels"])
    ap.add_argument("--batch2", type=int, default=30, help="stage-2 batch")
    ap.add_argument("--batch1", type=int, default=64, help="stage-1 batch")
    ap.add_argument("--steps", type=int, default=8, help="training steps per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per kernel timing")
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import torch

    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    rt.set_compute_dtype(opt.dtype)

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

    fmt = lambda v, u="ms": "  ".join(f"{x:8.3f}" for x in v) + f"   min {min(v):8.3f} {u}"
    lines = [f"weight EMA, part {opt.part}, {opt.dtype}, {torch.cuda.get_device_name(0)} (tools/ema_timing.py; HIP events, after warm-up, "
             f"{opt.rounds} alternating rounds)", ""]

    def step_block(name, tr, batches, warm):
        """off / on alternating on ONE trainer; `warm` untimed steps after every change (a recorded step is recorded again)"""
        step = [0]

        def steps(n):
            for _ in range(n):
                tr.train_step(batches[step[0] % len(batches)], step[0])
                step[0] += 1
        off, on = [], []
        for _ in range(opt.rounds):
            tr.set_weight_ema(0.0)
            steps(warm)
            r0 = tr.graph_replays
            off.append(timed(steps, opt.steps))
            off_replays = tr.graph_replays - r0
            tr.set_weight_ema(opt.decay, True)
            steps(warm)
            r0 = tr.graph_replays
            on.append(timed(steps, opt.steps))
            on_replays = tr.graph_replays - r0
        o = tr.opts[0]
        drift = float((o.flat_e - o.flat.flat_p).abs().max())
        oe, ne = [a for a, _ in off], [a for a, _ in on]
        oh, nh = [b for _, b in off], [b for _, b in on]
        lines.extend([
            f"(b) {name}: ms per training step, {opt.steps} steps per window (replayed steps per window: off {off_replays}, on {on_replays}); "
            f"flat sizes {[x.flat.flat_p.numel() for x in tr.opts]}:",
            f"  feature off,               HIP events   {fmt(oe)}",
            f"  ema_decay {opt.decay:g},          HIP events   {fmt(ne)}",
            f"  feature off,               host clock   {fmt(oh)}",
            f"  ema_decay {opt.decay:g},          host clock   {fmt(nh)}",
            f"  on - off (min over rounds): {min(ne) - min(oe):+.3f} ms HIP events ({(min(ne) / min(oe) - 1) * 100:+.2f} %), "
            f"{min(nh) - min(oh):+.3f} ms host clock; spread of the off windows {max(oe) - min(oe):.3f} ms",
            f"  last window: {o.ema_num_updates} EMA updates, decay of the last step {o._ema['last']:.6g}, max |e - p| {drift:.3g}",
            ""])

    if opt.part == "stage2":
        c = cfg.load_yaml(os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml"))
        model = cfg.instantiate_from_config(c.model).to(dev)
        model.learning_rate, model.min_learning_rate, model.training_steps, model.steps_per_epoch = 1e-5, 0.0, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=False)
        batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch2, 256, seed=300 + i)).to(dev)} for i in range(2)]
        step_block(f"stage 2, uncond_imagenet_p6c18.yml, batch {opt.batch2}, eager launches", tr, batches, 3)

    if opt.part == "stage1":
        yml = os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml")
        torch.manual_seed(0)
        model = cfg.instantiate_from_config(cfg.stage1_config(yml, batch_size=opt.batch1, objective="full").model).to(dev)
        model.learning_rate, model.training_steps, model.steps_per_epoch = 4.5e-6 * opt.batch1, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=True, graph_after=3)
        batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch1, 256, seed=1234 + 1000 * i)).to(dev)} for i in range(2)]
        step_block(f"stage 1, dqvae-entropy-dual-r05_imagenet.yml, batch {opt.batch1}, complete objective, recorded step", tr, batches, 6)

    if opt.part == "kernels":
        lines.append(f"(a) kernels alone, {opt.reps} calls per window; bytes/s = 12n / time for the EMA (reads e p, writes e), 16n / time for the "
                     "swap (reads and writes a b), 28n / time (reads p g m v, writes p m v) for Adam:")
        hyper = torch.zeros(8, dtype=torch.float32, device=dev)
        K.set_f32x8(hyper, [1e-5, 0.9, 0.95, 1e-8, 1.0, 1.0])
        rec = torch.zeros(8, dtype=torch.float32, device=dev)
        K.set_f32x8(rec, [1.0 - opt.decay])
        for name, n in SIZES.items():
            g = torch.randn(n, device=dev) * 1e-3
            p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            e = p.clone()

            def ema(reps):
                for _ in range(reps):
                    K.ema_update(e, p, rec)

            def swap(reps):
                for _ in range(reps):
                    K.swap_f32(e, p)

            def adam(reps):
                for _ in range(reps):
                    K.adamw_dev(p, g, m, v, hyper)
            for f in (ema, swap, adam):
                f(4)
            te, ts, ta = [], [], []
            for _ in range(opt.rounds):
                te.append(timed(ema, opt.reps)[0])
                ts.append(timed(swap, opt.reps)[0])
                ta.append(timed(adam, opt.reps)[0])
            re_, ra = 12 * n / (min(te) * 1e-3), 28 * n / (min(ta) * 1e-3)
            lines.extend([
                f"  {name}, n = {n} ({4 * n / 1e6:.1f} MB):",
                f"    dvq_ema_update       {fmt(te)}   {re_ / 1e12:.2f} TB/s   ({re_ / ra:.2f} of dvq_adamw_dev's rate)",
                f"    dvq_swap_f32         {fmt(ts)}   {16 * n / (min(ts) * 1e-3) / 1e12:.2f} TB/s",
                f"    dvq_adamw_dev        {fmt(ta)}   {ra / 1e12:.2f} TB/s"])
            del g, p, m, v, e
            torch.cuda.empty_cache()
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "a", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
