#!/usr/bin/env python3
"""Cost of classifier-free guidance (docs/design/14-guidance.md).

(a) the draw kernel: dvq_sample_guided at B = 32 pairs (64 logits rows), V = 2027, bf16, against dvq_sample_constrained at B = 32
    (content rule, top-k 300, multinomial), HIP events around `--reps` calls after a warm-up;
(b) images/s of the p6c18 class model (configs/stage2/class_imagenet_p6c18_cfg.yml, random weights, bf16) at batch 32, unguided
    (32 rows) and guided (32 pairs = 64 rows), on 1 and 4 lanes (Dualformer.sample_many): host clock around whole sampling calls
    that end in a synchronise, after every lane has captured its token-step graphs.  Token sampling only (no image decode).

Kernel times come from a run of their own: `rocprofv3 --kernel-trace --stats -f csv -d DIR -o guidance -- python
tools/guidance_timing.py --profile_only`, then `--kernel_stats DIR/.../guidance_kernel_stats.csv` adds its rows for the two kernels to the table.

    python tools/guidance_timing.py --out profiles/guidance_timing.txt [--kernel_stats stats.csv]
"""
import argparse
import csv
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def kernel_rows(path):
    """rows of a rocprofv3 kernel-stats CSV for the sampler kernels: (name, calls, average ns)"""
    out = []
    with open(path, newline="", encoding="utf-8") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "sample_constrained_kernel" in name:
                tag = "guided  " if ("Lb1E" in name or "true>" in name) else "unguided"
                out.append((f"{tag} {name[:90]}", int(r.get("Calls", 0)), float(r.get("AverageNs", 0.0))))
    return out


def draw_bench(dev, reps, profile_only):
    import torch

    from dynamicvectorquantization_amd import kernels as K
    b, v = 32, 2027
    g = torch.Generator(device="cpu").manual_seed(0)
    logits = (torch.randn(2 * b, v, generator=g) * 3).to(dev).to(torch.bfloat16)
    done = torch.zeros(2 * b, 1, device=dev)
    rule = dict(pad_code=1024, forbid_codes=(1024,), forbid_from=1025)
    st = torch.tensor([1, 0], dtype=torch.int64, device=dev)

    def unguided():
        K.sample_constrained(logits[:b], 1.0, state=st, finished=done[:b], top_k=300, sample=True, **rule)

    def guided():
        K.sample_guided(logits, 2.0, 1.0, state=st, finished=done, top_k=300, sample=True, **rule)

    for fn in (unguided, guided):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    if profile_only:
        for _ in range(reps):
            unguided()
            guided()
        torch.cuda.synchronize()
        return None

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps * 1e3           # us per call (draw + counter bump)

    res = {}
    for rnd in range(3):                                         # alternate the two: other work shares the host
        for name, fn in (("unguided", unguided), ("guided", guided)):
            res.setdefault(name, []).append(timed(fn))
    return res


def sampler_bench(dev, batches_per_lane):
    import torch

    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import runtime as rt
    rt.set_compute_dtype("bf16")
    torch.manual_seed(0)
    model = cfg.instantiate_from_config(cfg.load_yaml(os.path.join(REPO, "configs/stage2/class_imagenet_p6c18_cfg.yml")).model)
    model = model.eval().to(dev)
    b = 32
    kw = dict(temperature=1.0, sample=True, top_k=300, top_k_pos=1024, top_p=1.0, top_p_pos=1.0, process=False, fix_fine_position=False)
    rows = []
    for lanes in (1, 4):
        for guided in (False, True):
            n = lanes * batches_per_lane
            labels = [torch.arange(i * b, (i + 1) * b, device=dev) % model.n_classes for i in range(n)]
            conds = [model.guided_conditioning(l) if guided else model.encode_to_c(l) for l in labels]
            extra = dict(cfg_scale=2.0) if guided else {}
            model.sample_many(conds[:lanes], n_streams=lanes, **kw, **extra)        # every lane captures its graphs (alone)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = model.sample_many(conds, n_streams=lanes, **kw, **extra)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            tokens = sum(int(o[0].shape[0]) * int(o[0].shape[1] + o[1].shape[1]) for o in outs)
            rows.append((lanes, guided, n * b, dt, n * b / dt, tokens / (n * b)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--batches_per_lane", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel_stats", default="", help="rocprofv3 --stats kernel CSV of a --profile_only run")
    ap.add_argument("--profile_only", action="store_true")
    ap.add_argument("--skip_sampler", action="store_true")
    opt = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    res = draw_bench(dev, opt.reps, opt.profile_only)
    if opt.profile_only:
        print("profile run done")
        return
    lines = [f"classifier-free guidance cost, {torch.cuda.get_device_name(0)} (tools/guidance_timing.py)", "",
             "(a) one draw, V = 2027, bf16 logits, content rule, top-k 300, multinomial; HIP events over "
             f"{opt.reps} calls after a warm-up, three alternating rounds (us per call, incl. the counter bump)"]
    for name, label in (("unguided", "dvq_sample_constrained, B = 32 rows  "), ("guided", "dvq_sample_guided, B = 32 pairs      ")):
        t = res[name]
        lines.append(f"  {label} " + "  ".join(f"{x:7.2f}" for x in t) + f"   min {min(t):7.2f} us")
    lines.append(f"  guided / unguided (min over rounds): {min(res['guided']) / min(res['unguided']):.3f}x")
    if opt.kernel_stats:
        lines += ["", "  rocprofv3 --kernel-trace --stats (a --profile_only run of its own): kernel time"]
        for name, calls, avg in kernel_rows(opt.kernel_stats):
            lines.append(f"    {name}: {calls} calls, {avg / 1e3:.2f} us average")
    if not opt.skip_sampler:
        rows = sampler_bench(dev, opt.batches_per_lane)
        lines += ["", "(b) p6c18 class model (class_imagenet_p6c18_cfg.yml, random weights, bf16), batch 32, top-k 300 / 1024, "
                  "multinomial, token sampling only (host clock around sample_many + synchronise, lanes warm)"]
        for lanes, guided, n, dt, ips, tpi in rows:
            lines.append(f"  {lanes} lane{'s' if lanes > 1 else ' '}  {'guided s=2 (64 rows)' if guided else 'unguided  (32 rows)  '}  "
                         f"{n:4d} images in {dt:7.2f} s = {ips:7.2f} images/s   ({tpi:.0f} token steps per image, "
                         f"{ips * tpi:8.0f} image token-steps/s)")
        by = {(r[0], r[1]): r for r in rows}
        lines.append("  (the draws differ, so the sequence lengths do: token-steps/s compares equal work)")
        for lanes in (1, 4):
            g_, u_ = by[(lanes, True)], by[(lanes, False)]
            lines.append(f"  {lanes} lane{'s' if lanes > 1 else ''}: guided / unguided images/s = {g_[4] / u_[4]:.3f}, "
                         f"token-steps/s = {g_[4] * g_[5] / (u_[4] * u_[5]):.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
