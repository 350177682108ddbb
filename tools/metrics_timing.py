#!/usr/bin/env python3
"""What the training metric logs cost (docs/design/22-metrics-logging.md).

ms per training step with the logger off against on -- `csv`, a row every --every steps -- on ONE trainer in one process: the headline
stage-1 step (the benchmark's DQ-VAE, bf16, complete objective, the step recorded and replayed).  HIP events and the host clock up to the
synchronise, after a warm-up, alternating rounds, median and minimum over the rounds (docs/design/07-measurement.md), plus the number of
launches of the recorded step in both states.  A window is --steps steps long and holds steps // every row reads.

    python tools/metrics_timing.py --out profiles/metrics_timing.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50, help="training steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--every", type=int, default=50, help="log_every_n_steps of the logger")
    ap.add_argument("--writers", default="csv")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import torch

    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.metrics import MetricsLogger
    from dynamicvectorquantization_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    rt.set_compute_dtype(opt.dtype)

    def timed(fn, n):
        """(ms per step by HIP events, ms per step on the host clock up to the synchronise)"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        fn(n)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n, (time.perf_counter() - t0) * 1e3 / n

    yml = os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml")
    torch.manual_seed(0)
    model = cfg.instantiate_from_config(cfg.stage1_config(yml, batch_size=opt.batch, objective="full").model).to(dev)
    model.learning_rate, model.training_steps, model.steps_per_epoch = 4.5e-6 * opt.batch, 100000, 1000
    model.train()
    logdir = tempfile.mkdtemp(prefix="metrics_timing_")
    lg = MetricsLogger(logdir, writers=tuple(w for w in opt.writers.split(",") if w), log_every_n_steps=opt.every)
    tr = Trainer(model, max_steps=100000, use_graph=True, graph_after=3, metrics_logger=lg)
    batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch, 256, seed=1234 + 1000 * i)).to(dev)} for i in range(2)]
    step = [0]

    def steps(n):
        for _ in range(n):
            tr.train_step(batches[step[0] % len(batches)], step[0])
            step[0] += 1

    off, on, launches = [], [], {}
    for _ in range(opt.rounds):
        for name, logger, acc in (("off", None, off), ("on", lg, on)):
            tr.metrics_logger = logger          # another signature: the step is recorded again during the warm-up
            steps(6)
            launches[name] = tr._graph["sg"].launch_counts() if tr._graph else None
            r0 = tr.graph_replays
            acc.append(timed(steps, opt.steps))
            launches[name + "_replays"] = tr.graph_replays - r0
    rows = lg.rows_written
    lg.close()
    import shutil
    shutil.rmtree(logdir, ignore_errors=True)
    fmt = lambda v: "  ".join(f"{x:8.3f}" for x in v) + f"   median {statistics.median(v):8.3f}  min {min(v):8.3f} ms"
    oe, ne = [a for a, _ in off], [a for a, _ in on]
    oh, nh = [b for _, b in off], [b for _, b in on]
    d_ev, d_host = statistics.median(ne) - statistics.median(oe), statistics.median(nh) - statistics.median(oh)
    lines = [
        f"metric logs, stage 1 ({os.path.basename(yml)}, batch {opt.batch}, {opt.dtype}, complete objective, recorded step), "
        f"{torch.cuda.get_device_name(0)} (tools/metrics_timing.py; after warm-up, {opt.rounds} alternating rounds, {opt.steps} steps per window, "
        f"logger {opt.writers} with a row every {opt.every} steps)", "",
        f"  launches of the recorded step (kernels, of those on the side stream, cross-stream waits): off {launches.get('off')}, "
        f"on {launches.get('on')}; replayed steps per window: off {launches.get('off_replays')}, on {launches.get('on_replays')}",
        f"  logger off,   HIP events   {fmt(oe)}",
        f"  logger on,    HIP events   {fmt(ne)}",
        f"  logger off,   host clock   {fmt(oh)}",
        f"  logger on,    host clock   {fmt(nh)}",
        f"  on - off (medians): {d_ev:+.3f} ms HIP events ({d_ev / statistics.median(oe) * 100:+.2f} %), {d_host:+.3f} ms host clock; "
        f"spread of the off windows {max(oe) - min(oe):.3f} ms HIP events, {max(oh) - min(oh):.3f} ms host clock",
        f"  {rows} rows written, {len(lg.columns)} columns: {', '.join(lg.columns)}", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "a", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
