#!/usr/bin/env python3
"""What global-norm clipping and the non-finite guard cost (docs/design/19-gradient-clipping.md).

HIP events after a warm-up, alternating rounds in one process, minimum over the rounds (docs/design/07-measurement.md):
  (a) dvq_grad_sqnorm (both launches) on buffers of the stage-2 and the stage-1 optimizers' flat sizes: ms per call, bytes/s over the
      4n bytes it has to read, and dvq_adamw_dev against dvq_adamw_clip_dev on the same sizes
  (b) ms per training step with the feature off against clipping + guard on, same Trainer, same process:
      stage 2 (configs/stage2/uncond_imagenet_p6c18.yml, bf16, batch 30, eager launches) and
      stage 1 (the benchmark's DQ-VAE, bf16, complete objective, the step recorded and replayed)
Writes the table to --out (and prints it).

    python tools/gradclip_timing.py --out profiles/gradclip_timing.txt
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch2", type=int, default=30, help="stage-2 batch")
    ap.add_argument("--batch1", type=int, default=64, help="stage-1 batch")
    ap.add_argument("--steps", type=int, default=8, help="training steps per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per kernel timing")
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--skip-stage1", action="store_true")
    ap.add_argument("--skip-stage2", action="store_true")
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
    lines = [f"global-norm gradient clipping + non-finite guard, {opt.dtype}, {torch.cuda.get_device_name(0)} (tools/gradclip_timing.py; "
             f"HIP events, after warm-up, {opt.rounds} alternating rounds)", ""]
    sizes = {}

    def step_block(name, tr, batches, warm):
        """off / on alternating on ONE trainer; `warm` untimed steps after every change (a recorded step is recorded again)"""
        step = [0]

        def steps(n):
            for _ in range(n):
                tr.train_step(batches[step[0] % len(batches)], step[0])
                step[0] += 1
        off, on = [], []
        for _ in range(opt.rounds):
            tr.set_grad_guard(0.0, False)
            steps(warm)
            r0 = tr.graph_replays
            off.append(timed(steps, opt.steps))
            off_replays = tr.graph_replays - r0
            tr.set_grad_guard(opt.clip, True)
            steps(warm)
            r0 = tr.graph_replays
            on.append(timed(steps, opt.steps))
            on_replays = tr.graph_replays - r0
        stats = tr.grad_stats()
        oe, ne = [a for a, _ in off], [a for a, _ in on]
        oh, nh = [b for _, b in off], [b for _, b in on]
        lines.extend([
            f"(b) {name}: ms per training step, {opt.steps} steps per window (replayed steps per window: off {off_replays}, on {on_replays}):",
            f"  feature off,               HIP events   {fmt(oe)}",
            f"  clip {opt.clip:g} + guard on,       HIP events   {fmt(ne)}",
            f"  feature off,               host clock   {fmt(oh)}",
            f"  clip {opt.clip:g} + guard on,       host clock   {fmt(nh)}",
            f"  on - off (min over rounds): {min(ne) - min(oe):+.3f} ms HIP events ({(min(ne) / min(oe) - 1) * 100:+.2f} %), "
            f"{min(nh) - min(oh):+.3f} ms host clock; spread of the off windows {max(oe) - min(oe):.3f} ms",
            "  last step: " + "; ".join(f"opt{i} gnorm={s['norm']:.4g} coef={s['coef']:.4g} skipped={s['skipped']}" for i, s in enumerate(stats) if s),
            ""])

    if not opt.skip_stage2:
        c = cfg.load_yaml(os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml"))
        model = cfg.instantiate_from_config(c.model).to(dev)
        model.learning_rate, model.min_learning_rate, model.training_steps, model.steps_per_epoch = 1e-5, 0.0, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=False)
        sizes["stage 2 (StackGPT p6c18)"] = [o.flat.flat_g.numel() for o in tr.opts]
        batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch2, 256, seed=300 + i)).to(dev)} for i in range(2)]
        step_block(f"stage 2, uncond_imagenet_p6c18.yml, batch {opt.batch2}, eager launches", tr, batches, 3)
        del tr, model, batches
        torch.cuda.empty_cache()

    if not opt.skip_stage1:
        yml = os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml")
        torch.manual_seed(0)
        model = cfg.instantiate_from_config(cfg.stage1_config(yml, batch_size=opt.batch1, objective="full").model).to(dev)
        model.learning_rate, model.training_steps, model.steps_per_epoch = 4.5e-6 * opt.batch1, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=True, graph_after=3)
        sizes["stage 1 (DQ-VAE dual-grain, generator / discriminator)"] = [o.flat.flat_g.numel() for o in tr.opts]
        batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch1, 256, seed=1234 + 1000 * i)).to(dev)} for i in range(2)]
        step_block(f"stage 1, dqvae-entropy-dual-r05_imagenet.yml, batch {opt.batch1}, complete objective, recorded step", tr, batches, 6)
        del tr, model, batches
        torch.cuda.empty_cache()

    # ---- (a) the kernels alone, on buffers of the optimizers' sizes
    lines.append(f"(a) kernels alone, {opt.reps} calls per window; bytes/s = 4n / time for the norm, 28n / time (reads p g m v, writes p m v) for Adam:")
    hyper = torch.zeros(8, dtype=torch.float32, device=dev)
    K.set_f32x8(hyper, [1e-5, 0.9, 0.95, 1e-8, 1.0, 1.0])
    for name, ns in sizes.items():
        for n in ns:
            g = torch.randn(n, device=dev) * 1e-3
            p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            ws = torch.empty(K.grad_sqnorm_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
            gstat = K.grad_stats_block(dev)

            def norm(reps):
                for _ in range(reps):
                    K.grad_sqnorm(g, ws, gstat, opt.clip, True)

            def adam(reps):
                for _ in range(reps):
                    K.adamw_dev(p, g, m, v, hyper)

            def adam_clip(reps):
                for _ in range(reps):
                    K.adamw_clip_dev(p, g, m, v, hyper, gstat)
            for f in (norm, adam, adam_clip):
                f(3)
            tn, ta, tc = [], [], []
            for _ in range(opt.rounds):
                tn.append(timed(norm, opt.reps)[0])
                ta.append(timed(adam, opt.reps)[0])
                tc.append(timed(adam_clip, opt.reps)[0])
            want = float(g.double().norm())
            got = K.read_grad_stats(gstat)["norm"]
            lines.extend([
                f"  {name}, n = {n} ({4 * n / 1e6:.1f} MB), {len(ws)} partials; norm {got:.12g} (torch fp64 {want:.12g}):",
                f"    dvq_grad_sqnorm      {fmt(tn)}   {4 * n / (min(tn) * 1e-3) / 1e12:.2f} TB/s",
                f"    dvq_adamw_dev        {fmt(ta)}   {28 * n / (min(ta) * 1e-3) / 1e12:.2f} TB/s",
                f"    dvq_adamw_clip_dev   {fmt(tc)}   {28 * n / (min(tc) * 1e-3) / 1e12:.2f} TB/s"])
            del g, p, m, v, ws
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
