#!/usr/bin/env python3
"""What a training-time log event costs (docs/design/18-image-logging.md).  One GPU visit; kernel times by HIP events after a warm-up,
minimum over alternating rounds (docs/design/07-measurement.md); host times by perf_counter.
  (a) at the real size -- configs/stage1/dqvae-entropy-dual-r05_imagenet.yml, 16 images of 256 x 256, bf16 -- the GPU time of the panel
      kernels (two colour overlays) and of the four grid kernels, next to the eval forward they accompany
  (b) the host-blocking time of ImageLogger.maybe_log as the training loop sees it (no synchronisation; the writer's queue empty), and
      the time until its pictures are on disk
  (c) the reference's way on the same tensors: fp32 panels copied to the host, then tests/imagelog_cpu.py (numpy; the reference's PIL
      loops are slower still)
  (d) Trainer.fit -- the loop train.py runs -- over 200 steps after 20 warm-up steps, with a picture every 50 batches against none,
      alternating windows on one model: stage 1 (full objective, the YAML's batch size) and stage 2 (configs/stage2/uncond_imagenet_p6c18.yml,
      where the two sampling passes dominate the event: their share is reported)
Writes the table to --out (and prints it).

    python tools/imagelog_timing.py --out profiles/imagelog_timing.txt
"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--no-stage2", action="store_true")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import torch

    import imagelog_cpu as IC
    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import imagelog as IL
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.trainer import Trainer, reference_learning_rate
    dev = torch.device("cuda:0")
    rt.set_compute_dtype("bf16")
    torch.manual_seed(2021)
    lines = [f"training-time image logging, {torch.cuda.get_device_name(0)} (tools/imagelog_timing.py; bf16; kernel times: HIP events after "
             f"warm-up, {opt.rounds} alternating rounds of {opt.reps} calls, minimum)", ""]

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    def timed(fn, reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    def rounds(fns, reps):
        for f in fns.values():
            for _ in range(3):
                f()
        out = {n: [] for n in fns}
        for _ in range(opt.rounds):
            for n, f in fns.items():
                out[n].append(timed(f, reps))
        return {n: min(v) for n, v in out.items()}

    def build(yaml_path, bs):
        c = cfg.load_yaml(os.path.join(REPO, yaml_path))
        model = cfg.instantiate_from_config(c.model).to(dev)
        bs = bs or int(c.data.params.batch_size)
        model.steps_per_epoch, model.training_steps, model.max_epoch = 1000000, 1000000, 1
        model.learning_rate = reference_learning_rate(c.model, 1, bs)
        model.min_learning_rate = c.model.get("min_learning_rate", 0.)
        return model, bs

    # ---- (a) - (c): one event at the real size ----------------------------------------------------------------------------------------
    yaml1 = "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"
    model, bs1 = build(yaml1, None)
    model.train()
    x16 = torch.from_numpy(synth.half_flat_images(16, 256, seed=7)).to(dev)
    batch16 = {"image": x16}
    model.eval()
    with torch.no_grad():
        log = model.log_images(batch16)
        out = model._forward5(x16)
    grain, score = out[2].contiguous(), IL.normalize_scores(out[4]).contiguous()
    ws_b, ws_1 = K.imagelog_workspace(16, dev), K.imagelog_workspace(1, dev)
    o = torch.empty_like(x16)
    gbuf = torch.empty(K.image_grid_shape(16, 256, 256) + (3,), dtype=torch.uint8, device=dev)

    def fwd():
        with torch.no_grad():
            model._forward5(x16)
    r = rounds({
        "eval forward, 16 images (what the event is made of)": fwd,
        "dvq_grain_overlay, grain map (min/max + compose)": lambda: K.grain_overlay(x16, grain=grain, levels=2, scaler=0.7, ws=ws_b, out=o),
        "dvq_grain_overlay, entropy scores": lambda: K.grain_overlay(x16, score=score, scaler=0.7, ws=ws_b, out=o),
        "dvq_grain_lines (triple form of the map, in place)": lambda: K.grain_lines_(o, grain, 3),
        "dvq_image_grid_u8, one panel (min/max + compose)": lambda: K.image_grid_u8(x16, ws=ws_1, out=gbuf),
    }, opt.reps)
    say(f"(a) one log event at {yaml1}, 16 images of 256 x 256 ({x16.numel() * 4 / 1e6:.1f} MB per fp32 panel; grid {tuple(gbuf.shape)}):")
    for n, v in r.items():
        say(f"  {n:62s} {v:9.4f} ms")
    kern = r["dvq_grain_overlay, grain map (min/max + compose)"] + r["dvq_grain_overlay, entropy scores"] + \
        4 * r["dvq_image_grid_u8, one panel (min/max + compose)"]
    fw = r["eval forward, 16 images (what the event is made of)"]
    say(f"  panel + grid kernels of the event (2 overlays + 4 grids): {kern:.4f} ms = {kern / fw:.4f} of the eval forward")
    say()

    tmp = tempfile.mkdtemp(prefix="dvq_imagelog_")
    lg = IL.ImageLogger(tmp, batch_frequency=1, max_images=16)
    model.train()
    host, gpu, disk = [], [], []
    for i in range(6):
        lg.flush()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        lg.maybe_log(model, batch16, i, "train")
        ev[1].record()
        t1 = time.perf_counter()
        lg.flush()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        if i:                                   # the first call warms allocations and the writer
            host.append((t1 - t0) * 1e3)
            gpu.append(ev[0].elapsed_time(ev[1]))
            disk.append((t2 - t0) * 1e3)
    say("(b) ImageLogger.maybe_log on that model and batch (5 events after one warm-up; writer queue empty before each):")
    say(f"  host time the training loop is blocked (no synchronisation)   " + "  ".join(f"{v:8.3f}" for v in host) + f"   min {min(host):8.3f} ms")
    say(f"  GPU time it puts on the training stream (eval forward + panels) " + "  ".join(f"{v:8.3f}" for v in gpu) + f"   min {min(gpu):8.3f} ms")
    say(f"  until the four PNGs are on disk (grids, copies, encoding)       " + "  ".join(f"{v:8.3f}" for v in disk) + f"   min {min(disk):8.3f} ms")
    say()

    cpu = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_panels = {k: v[:16].detach().cpu().numpy() for k, v in (("inputs", x16), ("reconstructions", log["reconstructions"]))}
        g_np, s_np = grain.cpu().numpy(), score.cpu().numpy()
        t1 = time.perf_counter()
        host_panels["grain_map"] = IC.overlay(host_panels["inputs"], grain=g_np, levels=2, scaler=0.7)
        host_panels["entropy_map"] = IC.overlay(host_panels["inputs"], score=s_np, scaler=0.7)
        t2 = time.perf_counter()
        for v in host_panels.values():
            IC.grid_u8(v, nrow=4, padding=2, clamp=True)
        t3 = time.perf_counter()
        cpu.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    best = min(cpu, key=sum)
    say("(c) the host's way on the same tensors (tests/imagelog_cpu.py, numpy; best of 3):")
    say(f"  device-to-host copy of the fp32 inputs / reconstructions and the maps {best[0]:9.3f} ms")
    say(f"  two colour overlays                                                   {best[1]:9.3f} ms")
    say(f"  four grids                                                            {best[2]:9.3f} ms")
    say(f"  total {sum(best):.3f} ms of a stalled training loop, against {min(host):.3f} ms blocked and {kern:.4f} ms of kernels above")
    say()
    del lg, log, out
    model = None
    torch.cuda.empty_cache()

    # ---- (d) throughput of the fit loop --------------------------------------------------------------------------------------------
    def throughput(label, yaml_path, bs, windows=("off", "on", "off", "on")):
        model, bs = build(yaml_path, bs)
        pool = [torch.from_numpy(synth.half_flat_images(bs, 256, seed=40 + i)).to(dev) for i in range(4)]
        key = getattr(model, "image_key", None) or getattr(model, "first_stage_key", "image")
        tr = Trainer(model, max_steps=0)
        marks = {}

        def batch_fn(step):
            if step == marks["start"]:
                torch.cuda.synchronize()
                marks["t0"] = time.perf_counter()
            return {key: pool[step % 4]}
        res = {"off": [], "on": []}
        events = 0
        for w in windows:
            first = int(model.global_step)
            marks["start"] = first + opt.warm
            tr.max_steps = first + opt.warm + opt.steps
            lgw = IL.ImageLogger(tempfile.mkdtemp(prefix="dvq_imagelog_"), batch_frequency=opt.every, max_images=16) if w == "on" else None
            tr.fit(batch_fn, image_logger=lgw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - marks["t0"]
            res[w].append(opt.steps * bs / dt)
            if lgw is not None:
                events = lgw.events
        say(f"(d) {label}: {yaml_path}, bs {bs}, Trainer.fit, {opt.steps} steps per window after {opt.warm} warm-up steps "
            f"(recorded-step replays: {tr.graph_replays}); windows alternate on one model; pictures every {opt.every} batches "
            f"({events} events in an `on` window, its last flush included):")
        for w in ("off", "on"):
            say(f"  logging {w:3s}  " + "  ".join(f"{v:9.2f}" for v in res[w]) + f"   max {max(res[w]):9.2f} img/s")
        say(f"  on / off: {max(res['on']) / max(res['off']):.4f}")
        return model, bs, pool, key

    model, bs, pool, key = throughput("stage 1", yaml1, bs1)
    say()
    del model, pool
    torch.cuda.empty_cache()
    if not opt.no_stage2:
        yaml2 = "configs/stage2/uncond_imagenet_p6c18.yml"
        model, bs, pool, key = throughput("stage 2", yaml2, None)
        lg = IL.ImageLogger(tempfile.mkdtemp(prefix="dvq_imagelog_"), batch_frequency=1, max_images=16)
        batch = {key: pool[0]}

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        flags = [(m, m.training) for m in model.modules()]
        model.eval()
        st = lg.sampler_state(dev)
        model.current_epoch = 1
        model.log_images(batch, sampler_state=st)                       # warm: K/V caches, captured token steps
        samples = min(wall(lambda: model.log_images(batch, sampler_state=st)) for _ in range(2))
        model.current_epoch = 0
        full = min(wall(lambda: model.log_images(batch, sampler_state=st)) for _ in range(2))
        for m, was in flags:
            m.training = was
        event = min(wall(lambda: (lg.maybe_log(model, batch, 0, "train"), lg.flush())) for _ in range(2))
        say(f"  one stage-2 event, synchronised: {event:.1f} ms in all; log_images {full:.1f} ms, of which the two sampling passes "
            f"(4 images each, decoded) {samples:.1f} ms = {samples / event:.3f} of the event")
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
