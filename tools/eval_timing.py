#!/usr/bin/env python3
"""Cost of the reconstruction evaluation next to the autoencoder forward it measures (docs/design/13-evaluation.md).

On one batch (default B = 64, 256 x 256, bf16, the shipped entropy-dual YAML with random weights), timed with HIP events after a
warm-up: dvq_recon_metrics + dvq_code_histogram against model.ae_fwd, and evaluate_reconstruction's images/s against a forward-only
loop over the same batches.  Writes the table to --out (and prints it).  --profile_only: a short run without the tables, for
`rocprofv3 --kernel-trace --stats -- python tools/eval_timing.py --profile_only` (kernel statistics in a run of their own).

    python tools/eval_timing.py --out profiles/eval_metrics_timing.txt
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batches", type=int, default=8, help="batches of the loop comparison")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--profile_only", action="store_true")
    opt = ap.parse_args()
    import torch

    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    dev = torch.device("cuda:0")
    rt.set_compute_dtype(opt.dtype)
    model, size = E.load_model(os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"), "", dev)
    size = opt.size
    k = model.quantize.codebook.n_embed
    xs = [torch.from_numpy(synth.half_flat_images(opt.batch, size, seed=100 + i)).to(dev) for i in range(opt.batches)]
    x = xs[0]
    counts = torch.zeros(model.N_GRAINS, k, dtype=torch.int64, device=dev)
    invalid = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = K.recon_metrics_workspace(opt.batch, size, size, dev)

    def metrics(out):
        K.recon_metrics(x, out["rec"], True, ws)
        K.code_histogram(out["codes"], out["grain"], k, model.N_GRAINS, counts, invalid)

    with torch.no_grad():
        out = model.ae_fwd(x, None)
        for _ in range(3):
            metrics(out)
        torch.cuda.synchronize()
        if opt.profile_only:
            E.evaluate_reconstruction(model, xs[:2], lpips=False)
            torch.cuda.synchronize()
            print("profile run done")
            return

        def timed(fn, reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / reps

        t_fwd = timed(lambda: model.ae_fwd(x, None), max(3, opt.reps // 4))
        t_rm = timed(lambda: K.recon_metrics(x, out["rec"], True, ws), opt.reps)
        t_ch = timed(lambda: K.code_histogram(out["codes"], out["grain"], k, model.N_GRAINS, counts, invalid), opt.reps)
        t_both = timed(lambda: metrics(out), opt.reps)

        def fwd_loop():
            for b in xs:
                model.ae_fwd(b, None)

        def eval_loop():
            E.evaluate_reconstruction(model, xs, lpips=False)

        fwd_loop()
        eval_loop()
        torch.cuda.synchronize()
        rates = {}
        for name, fn in (("forward only", fwd_loop), ("evaluate_reconstruction", eval_loop), ("forward only (again)", fwd_loop),
                         ("evaluate_reconstruction (again)", eval_loop)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates[name] = opt.batches * opt.batch / (time.perf_counter() - t0)
    n_img = opt.batch * 3 * size * size
    lines = [
        f"reconstruction-evaluation cost, B = {opt.batch}, {size} x {size}, {opt.dtype}, {torch.cuda.get_device_name(0)} "
        f"(tools/eval_timing.py; HIP events, after warm-up)",
        "",
        f"ae_fwd (one batch)                          {t_fwd:9.3f} ms",
        f"dvq_recon_metrics (tile + fold kernels)     {t_rm * 1e3:9.1f} us   ({2 * n_img * 4 / (t_rm * 1e-3) / 1e9:.0f} GB/s of input read)",
        f"dvq_code_histogram                          {t_ch * 1e3:9.1f} us",
        f"both, back to back                          {t_both * 1e3:9.1f} us   = {100 * t_both / t_fwd:.3f} % of ae_fwd",
        "",
        f"loop over {opt.batches} batches of {opt.batch} (host clock around work ending in a synchronise):",
    ]
    lines += [f"  {name:34s} {r:9.1f} images/s" for name, r in rates.items()]
    fo = min(rates["forward only"], rates["forward only (again)"])
    ev = max(rates["evaluate_reconstruction"], rates["evaluate_reconstruction (again)"])
    fo_best = max(rates["forward only"], rates["forward only (again)"])
    ev_worst = min(rates["evaluate_reconstruction"], rates["evaluate_reconstruction (again)"])
    lines.append(f"  evaluation loop vs forward only: {100 * (1 - ev_worst / fo_best):+.2f} % (worst pair) / "
                 f"{100 * (1 - ev / fo):+.2f} % (best pair) slower")
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
