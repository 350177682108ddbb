#!/usr/bin/env python3
"""What per-parameter norm tracking costs (docs/design/24-norm-tracking.md).

HIP events after a warm-up, alternating rounds in one process, minimum over the rounds (docs/design/07-measurement.md):
  (1) the gradient pass (dvq_segment_stats, sticky, both launches) on the flat buffers of the stage-2 and stage-1 optimizers with the
      real models' segment tables, against dvq_grad_sqnorm on the same buffer in the same process: ms per call, bytes/s over the 4n
      bytes either has to read, and the ratio
  (2) the armed trio of a row step -- snapshot copy, weight pass, update pass -- against three device copies of the buffer
  (3) ms per training step, tracking off against on with a row every --every steps, alternating windows of --steps steps on one
      Trainer: stage 2 (configs/stage2/uncond_imagenet_p6c18.yml, bf16, eager launches) and stage 1 (the benchmark's DQ-VAE, bf16,
      complete objective, the step recorded and replayed); the difference next to the spread of the off windows
  (4) with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 20 --warmup 5` there and here, alternating,
      --rounds rounds -- "off costs nothing" means this tree's figures lie inside the parent's own range
Writes the table to --out (and prints it).

    python tools/normtrack_timing.py --out profiles/normtrack_timing.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch2", type=int, default=30, help="stage-2 batch")
    ap.add_argument("--batch1", type=int, default=64, help="stage-1 batch")
    ap.add_argument("--steps", type=int, default=50, help="training steps per timed window")
    ap.add_argument("--every", type=int, default=50, help="a row step every N steps")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30, help="calls per kernel timing")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--skip-stage1", action="store_true")
    ap.add_argument("--skip-stage2", action="store_true")
    ap.add_argument("--skip-steps", action="store_true", help="(1) and (2) only: the models are built for their segment tables, no step is timed")
    ap.add_argument("--parent", default="", help="(4): a built checkout of the parent commit")
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
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        fn(n)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    fmt = lambda v, u="ms": "  ".join(f"{x:8.3f}" for x in v) + f"   min {min(v):8.3f} {u}"
    lines = [f"per-parameter norm tracking, {opt.dtype}, {torch.cuda.get_device_name(0)} (tools/normtrack_timing.py; HIP events, after "
             f"warm-up, {opt.rounds} alternating rounds)", ""]
    tables = {}                 # name -> list of offsets lists, one per optimizer

    def offsets_of(o):
        offs = [0]
        for p in o.flat.params:
            offs.append(offs[-1] + p.numel())
        return offs

    def step_block(name, tr, batches, warm):
        step = [0]

        def steps(n):
            for _ in range(n):
                tr.train_step(batches[step[0] % len(batches)], step[0])
                step[0] += 1
        off, on = [], []
        for _ in range(opt.rounds):
            tr.set_norm_tracking(-1)
            steps(warm)
            off.append(timed(steps, opt.steps))
            tr.set_norm_tracking(2, True)
            tr.norm_every = opt.every
            steps(warm)
            r0 = tr.graph_replays
            on.append(timed(steps, opt.steps))
            on_replays = tr.graph_replays - r0
        stats = tr.norm_stats()
        lines.extend([
            f"(3) {name}: ms per training step, {opt.steps} steps per window, a row every {opt.every} (replayed steps per on window: {on_replays}):",
            f"  tracking off   {fmt(off)}",
            f"  tracking on    {fmt(on)}",
            f"  on - off (min over rounds): {min(on) - min(off):+.3f} ms ({(min(on) / min(off) - 1) * 100:+.2f} %); spread of the off windows "
            f"{max(off) - min(off):.3f} ms",
            "  last row: " + "; ".join(f"opt{i}: {len(s)} parameters, largest update ratio {max(e['update_ratio'] for e in s.values()):.3g}"
                                       for i, s in enumerate(stats)),
            ""])
        tr.set_norm_tracking(-1)

    if not opt.skip_stage2:
        c = cfg.load_yaml(os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml"))
        model = cfg.instantiate_from_config(c.model).to(dev)
        model.learning_rate, model.min_learning_rate, model.training_steps, model.steps_per_epoch = 1e-5, 0.0, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=False)
        tables["stage 2 (StackGPT p6c18)"] = [offsets_of(o) for o in tr.opts]
        if not opt.skip_steps:
            batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch2, 256, seed=300 + i)).to(dev)} for i in range(2)]
            step_block(f"stage 2, uncond_imagenet_p6c18.yml, batch {opt.batch2}, eager launches", tr, batches, 3)
            del batches
        del tr, model
        torch.cuda.empty_cache()

    if not opt.skip_stage1:
        yml = os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml")
        torch.manual_seed(0)
        model = cfg.instantiate_from_config(cfg.stage1_config(yml, batch_size=opt.batch1, objective="full").model).to(dev)
        model.learning_rate, model.training_steps, model.steps_per_epoch = 4.5e-6 * opt.batch1, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=True, graph_after=3)
        tables["stage 1 (DQ-VAE dual-grain, generator / discriminator)"] = [offsets_of(o) for o in tr.opts]
        if not opt.skip_steps:
            batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch1, 256, seed=1234 + 1000 * i)).to(dev)} for i in range(2)]
            step_block(f"stage 1, dqvae-entropy-dual-r05_imagenet.yml, batch {opt.batch1}, complete objective, recorded step", tr, batches, 6)
            del batches
        del tr, model
        torch.cuda.empty_cache()

    lines.append(f"(1), (2) kernels alone, {opt.reps} calls per window; bytes/s = 4n / time for the two norm passes:")
    for name, tabs in tables.items():
        for offs in tabs:
            n, S = offs[-1], len(offs) - 1
            plan = K.SegmentPlan(offs, dev)
            g = torch.randn(n, device=dev) * 1e-3
            p = torch.randn(n, device=dev)
            snap, spare = torch.empty_like(p), torch.empty_like(p)
            ws = K.segment_stats_workspace(n, S, dev)
            sg, sw, su = (K.segment_stats_state(S, dev) for _ in range(3))
            ws1 = torch.empty(K.grad_sqnorm_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
            gstat = K.grad_stats_block(dev)
            armed = torch.ones(1, dtype=torch.int32, device=dev)
            aligned = sum(1 for o in offs[:-1] if o % 4 == 0)

            def seg(reps):
                for _ in range(reps):
                    K.segment_stats(g, None, plan, ws, sg, sticky=True)

            def whole(reps):
                for _ in range(reps):
                    K.grad_sqnorm(g, ws1, gstat, 0.0, True)

            def trio(reps):
                for _ in range(reps):
                    K.copy_f32_armed(snap, p, armed)
                    K.segment_stats(p, None, plan, ws, sw, armed=armed)
                    K.segment_stats(p, snap, plan, ws, su, armed=armed)

            def copies(reps):
                for _ in range(reps):
                    spare.copy_(p)
                    snap.copy_(p)
                    spare.copy_(p)

            def unarmed(reps):
                armed.zero_()
                trio(reps)
                armed.fill_(1)
            for f in (seg, whole, trio, copies, unarmed):
                f(3)
            ts, tw, tt, tc, tu = [], [], [], [], []
            for _ in range(opt.rounds):
                ts.append(timed(seg, opt.reps))
                tw.append(timed(whole, opt.reps))
                tt.append(timed(trio, opt.reps))
                tc.append(timed(copies, opt.reps))
                tu.append(timed(unarmed, opt.reps))
            total = float(torch.sqrt(K.segment_stats_views(sg.cpu(), S)["sumsq"].sum()))
            lines.extend([
                f"  {name}, n = {n} ({4 * n / 1e6:.1f} MB), {S} segments ({aligned} start on a 16-byte boundary), {plan.nchunks} chunks "
                f"(dvq_grad_sqnorm: {len(ws1)}); norm {total:.12g} (dvq_grad_sqnorm {K.read_grad_stats(gstat)['norm']:.12g}):",
                f"    (1) dvq_segment_stats, sticky     {fmt(ts)}   {4 * n / (min(ts) * 1e-3) / 1e12:.2f} TB/s",
                f"        dvq_grad_sqnorm               {fmt(tw)}   {4 * n / (min(tw) * 1e-3) / 1e12:.2f} TB/s   ratio {min(ts) / min(tw):.3f}",
                f"    (2) snapshot + weight + update    {fmt(tt)}   {20 * n / (min(tt) * 1e-3) / 1e12:.2f} TB/s over 20n bytes",
                f"        three device copies           {fmt(tc)}   {24 * n / (min(tc) * 1e-3) / 1e12:.2f} TB/s over 24n bytes   ratio {min(tt) / min(tc):.3f}",
                f"        the trio unarmed (5 launches) {fmt(tu)}"])
            del g, p, snap, spare, ws, ws1
            torch.cuda.empty_cache()

    if opt.parent:
        lines.extend(["", f"(4) bench.py --gpus 1 --steps 20 --warmup 5, parent checkout against this tree, alternating, {opt.rounds} rounds:"])
        res = {"parent": [], "this tree": []}
        failed = False
        for _ in range(opt.rounds):
            for tag, root in (("parent", os.path.abspath(opt.parent)), ("this tree", REPO)):
                if failed:                 # a benchmark that failed is not started again
                    break
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=root, capture_output=True,
                                   text=True, timeout=600)
                last = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                failed = r.returncode != 0 or not last
                res[tag].append({"error": r.returncode, "stderr": r.stderr[-400:]} if failed else json.loads(last[-1]))
                print(tag, f"{time.perf_counter() - t0:.0f} s", res[tag][-1], flush=True)
        for tag, rs in res.items():
            if any("error" in r for r in rs):
                lines.append(f"  {tag:10s} failed: " + "  ".join(json.dumps(r, sort_keys=True) for r in rs if "error" in r))
                continue
            launches = sorted({tuple(r["config"]["step_graph"].get("launches_main_side_waits") or ()) for r in rs})
            lines.append(f"  {tag:10s} images/sec " + "  ".join(f"{r['value']:8.2f}" for r in rs) + "   ms per step " +
                         "  ".join(f"{r['ms_per_step']:8.3f}" for r in rs) + f"   recorded launches (main, side, waits) {launches}")
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
