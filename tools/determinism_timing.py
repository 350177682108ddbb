#!/usr/bin/env python3
"""What deterministic mode costs (docs/design/21-reproducible-training.md).

HIP events after a warm-up, the two settings ALTERNATING in one process, every round listed (docs/design/07-measurement.md):
  --part stage1 / stage2: ms per training step with kernels.set_deterministic off against on, same Trainer, same process:
      stage 1 = the benchmark's DQ-VAE (configs/stage1/dqvae-entropy-dual-r05_imagenet.yml, bf16, batch 64, complete objective, the
      step recorded and replayed -- recorded again after every change of the mode), stage 2 = configs/stage2/uncond_imagenet_p6c18.yml
      (bf16, batch 30, eager launches)
  --part trace --stage N --det 0|1: nothing but warm-up + steps, to be run under the profiler, once per setting:
      rocprofv3 --kernel-trace --stats -d DIR -o det1 -- python tools/determinism_timing.py --part trace --stage 1 --det 1
  --part families --off STATS.csv --on STATS.csv --steps N: per-family kernel time per step from the two kernel_stats files of such
      runs (N = every step a run made, warm-up included: 6 + 8 for stage 1, 3 + 8 for stage 2)
Each part is one process; the table is appended to --out (and printed).
"""
import argparse
import csv
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# kernel name (as the profiler prints it) -> reduction family of docs/design/21-reproducible-training.md; first match wins
FAMILIES = [
    ("deterministic folds", r"det_fold_kernel|tn_det_fold_kernel"),
    ("GroupNorm / BatchNorm statistics", r"gn_stats_kernel"),
    ("GroupNorm / BatchNorm backward sums", r"gn_bwd_reduce_kernel|gn_bwd_finalize_kernel"),
    ("halo conv (+ statistics epilogue)", r"conv3x3_halo_kernel|halo_stats_finalize_kernel"),
    ("halo weight gradient", r"conv3x3_halo_wgrad"),
    ("TN weight gradients", r"igemm_tn|conv_tn_patch|gemm_tn_|naive_tn"),
    ("column / batch sums", r"sum_batch"),
    ("LayerNorm backward", r"ln_bwd"),
    ("embedding gradient", r"embed_scatter"),
    ("cross entropy", r"cross_entropy"),
    ("scalar loss sums", r"l1_loss_kernel|vq_gather_loss_kernel|lpips_head_kernel"),
    ("VQ-EMA statistics", r"vq_ema_stats_kernel"),
]


def family_table(off_csv, on_csv, steps):
    def read(path):
        tot = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
                fam = next((fam for fam, pat in FAMILIES if re.search(pat, name)), "everything else")
                tot[fam] = tot.get(fam, 0.0) + ns
        return tot
    off, on = read(off_csv), read(on_csv)
    lines = [f"per-family kernel time per step (ms; rocprofv3 --kernel-trace --stats, {steps} steps per run, one run per setting):",
             f"  {'family':40s} {'off':>10s} {'on':>10s} {'on - off':>10s}"]
    for fam in [f for f, _ in FAMILIES] + ["everything else"]:
        a, b = off.get(fam, 0.0) / steps / 1e6, on.get(fam, 0.0) / steps / 1e6
        if a or b:
            lines.append(f"  {fam:40s} {a:10.3f} {b:10.3f} {b - a:+10.3f}")
    ta, tb = sum(off.values()) / steps / 1e6, sum(on.values()) / steps / 1e6
    lines.append(f"  {'all kernels':40s} {ta:10.3f} {tb:10.3f} {tb - ta:+10.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["stage1", "stage2", "trace", "families"])
    ap.add_argument("--stage", type=int, default=1, help="--part trace: 1 | 2")
    ap.add_argument("--det", type=int, default=0, help="--part trace: the mode of the run")
    ap.add_argument("--off", default="", help="--part families: kernel_stats.csv of the run with the mode off")
    ap.add_argument("--on", default="", help="--part families: kernel_stats.csv of the run with the mode on")
    ap.add_argument("--batch1", type=int, default=64)
    ap.add_argument("--batch2", type=int, default=30)
    ap.add_argument("--steps", type=int, default=8, help="training steps per timed window")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()

    def emit(lines):
        text = "\n".join(lines) + "\n"
        print(text)
        if opt.out:
            with open(opt.out, "a", encoding="utf-8") as f:
                f.write(text)

    if opt.part == "families":
        emit(family_table(opt.off, opt.on, opt.steps) + [""])
        return
    import torch

    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    rt.set_compute_dtype(opt.dtype)
    K.ensure_workspace(dev)
    stage = int(opt.part[-1]) if opt.part != "trace" else opt.stage
    torch.manual_seed(0)
    if stage == 1:
        yml = os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml")
        model = cfg.instantiate_from_config(cfg.stage1_config(yml, batch_size=opt.batch1, objective="full").model).to(dev)
        model.learning_rate, model.training_steps, model.steps_per_epoch = 4.5e-6 * opt.batch1, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=True, graph_after=3)
        batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch1, 256, seed=1234 + 1000 * i)).to(dev)} for i in range(2)]
        name, warm = f"stage 1, dqvae-entropy-dual-r05_imagenet.yml, batch {opt.batch1}, complete objective, recorded step", 6
    else:
        c = cfg.load_yaml(os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml"))
        model = cfg.instantiate_from_config(c.model).to(dev)
        model.learning_rate, model.min_learning_rate, model.training_steps, model.steps_per_epoch = 1e-5, 0.0, 100000, 1000
        model.train()
        tr = Trainer(model, max_steps=100000, use_graph=False)
        batches = [{"image": torch.from_numpy(synth.half_flat_images(opt.batch2, 256, seed=300 + i)).to(dev)} for i in range(2)]
        name, warm = f"stage 2, uncond_imagenet_p6c18.yml, batch {opt.batch2}, eager launches", 3
    step = [0]

    def steps(n):
        for _ in range(n):
            tr.train_step(batches[step[0] % len(batches)], step[0])
            step[0] += 1

    def timed(n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        steps(n)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n, (time.perf_counter() - t0) * 1e3 / n

    if opt.part == "trace":
        K.set_deterministic(bool(opt.det))
        steps(warm)
        torch.cuda.synchronize()
        c0 = K.unordered_launches()
        steps(opt.steps)
        torch.cuda.synchronize()
        print(f"[determinism_timing] trace run: {name}, deterministic {bool(opt.det)}, {warm} + {opt.steps} steps, "
              f"{K.unordered_launches() - c0} unordered launches in the last {opt.steps}")
        return
    fmt = lambda v: "  ".join(f"{x:8.3f}" for x in v) + f"   min {min(v):8.3f}  median {sorted(v)[len(v) // 2]:8.3f} ms"
    off, on, counts = [], [], {}
    try:
        for _ in range(opt.rounds):
            for det, dst in ((False, off), (True, on)):
                K.set_deterministic(det)
                tr.drop_graph()
                steps(warm)
                c0, r0 = K.unordered_launches(), tr.graph_replays
                dst.append(timed(opt.steps))
                counts[det] = (K.unordered_launches() - c0, tr.graph_replays - r0)
    finally:
        K.set_deterministic(False)
    oe, ne = [a for a, _ in off], [a for a, _ in on]
    oh, nh = [b for _, b in off], [b for _, b in on]
    emit([
        f"deterministic mode, part {opt.part}, {opt.dtype}, {torch.cuda.get_device_name(0)} (tools/determinism_timing.py; HIP events, "
        f"after warm-up, {opt.rounds} alternating rounds)", "",
        f"{name}: ms per training step, {opt.steps} steps per window",
        f"  (per window: unordered launches off {counts[False][0]}, on {counts[True][0]}; replayed steps off {counts[False][1]}, on {counts[True][1]})",
        f"  mode off,   HIP events   {fmt(oe)}",
        f"  mode on,    HIP events   {fmt(ne)}",
        f"  mode off,   host clock   {fmt(oh)}",
        f"  mode on,    host clock   {fmt(nh)}",
        f"  on - off (min over rounds): {min(ne) - min(oe):+.3f} ms HIP events ({(min(ne) / min(oe) - 1) * 100:+.2f} %); "
        f"spread of the off windows {max(oe) - min(oe):.3f} ms, of the on windows {max(ne) - min(ne):.3f} ms", ""])


if __name__ == "__main__":
    main()
