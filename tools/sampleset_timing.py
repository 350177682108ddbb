#!/usr/bin/env python3
"""Cost of the sample-set metrics' device passes (docs/design/32-sample-set-metrics.md).

N = M = 10 000 and 50 000 rows of D = 1024 structured features, k = 5; one process, HIP events after a warm-up.  Per size: the four
scans of evaluate.sample_set_metrics (R|R and F|F without the diagonal, F|R and R|F with radii) and the two moment passes, the scans'
achieved FLOP/s (2 N M D per scan) against the fp32 matrix-instruction peak, and -- alternating with the kernel in the same process --
the ATen composition of one scan: chunked fp32 torch.mm + row norms + topk, the chunk sized so that its N x chunk temporaries fit.
Writes the table to --out.

    python tools/sampleset_timing.py --out profiles/sampleset_timing.txt
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

PEAK_F32_MFMA_TFLOPS = 157.3        # v_mfma_f32_32x32x2_f32 at 64 FLOP / clk / SIMD, MI355X spec sheet (= the fp32 vector peak)


def aten_scan(a, b, k, rad2_b, chunk):
    """the same outputs from library calls: per chunk of b an [Na, chunk] distance block (never the whole matrix), a running top-k"""
    import torch
    na2 = (a * a).sum(dim=1, keepdim=True)
    best_d = torch.full((a.shape[0], k), float("inf"), device=a.device)
    best_i = torch.full((a.shape[0], k), -1, dtype=torch.long, device=a.device)
    count = torch.zeros(a.shape[0], dtype=torch.long, device=a.device)
    for j0 in range(0, b.shape[0], chunk):
        bj = b[j0:j0 + chunk]
        d2 = (na2 + (bj * bj).sum(dim=1)[None, :] - 2.0 * torch.mm(a, bj.t())).clamp_(min=0.0)
        count += (d2 <= rad2_b[None, j0:j0 + chunk]).sum(dim=1)
        d, i = torch.topk(d2, min(k, d2.shape[1]), dim=1, largest=False)
        cat_d, cat_i = torch.cat([best_d, d], dim=1), torch.cat([best_i, i + j0], dim=1)
        best_d, sel = torch.topk(cat_d, k, dim=1, largest=False)
        best_i = torch.gather(cat_i, 1, sel)
    return best_d, best_i, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4096, help="rows of b per ATen block (50 000 x 4096 fp32 = 0.8 GB per temporary)")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import torch

    import sampleset_math as SM
    from dynamicvectorquantization_amd import kernels as K
    dev = torch.device("cuda:0")

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    lines = [f"sample-set metric passes, D = {opt.dim}, k = {opt.k}, {torch.cuda.get_device_name(0)} (tools/sampleset_timing.py; HIP events, "
             f"after a warm-up, best of {opt.rounds} rounds, one process; ATen: fp32 torch.mm + topk over blocks of {opt.chunk} rows of b)", ""]
    for n in opt.sizes:
        real, fake = SM.make_sets(n, n, opt.dim, seed=n)
        xr, xf = (torch.from_numpy(v).to(dev) for v in SM.centre(real, fake))
        zero = torch.zeros(opt.dim, device=dev)
        k = opt.k
        rad_r = K.pair_scan(xr, xr, k, exclude_diag=True)[0][:, k - 1].contiguous()
        rad_f = K.pair_scan(xf, xf, k, exclude_diag=True)[0][:, k - 1].contiguous()
        ws = K.pair_scan_workspace(n, n, k, dev)
        fns = {"scan R|R (no diagonal)": lambda: K.pair_scan(xr, xr, k, exclude_diag=True, ws=ws),
               "scan F|F (no diagonal)": lambda: K.pair_scan(xf, xf, k, exclude_diag=True, ws=ws),
               "scan F|R (radii)": lambda: K.pair_scan(xf, xr, k, rad2_b=rad_r, ws=ws),
               "scan R|F (radii)": lambda: K.pair_scan(xr, xf, k, rad2_b=rad_f, ws=ws),
               "ATen  F|R (radii)": lambda: aten_scan(xf, xr, k, rad_r, opt.chunk),
               "moments R": lambda: K.feat_moments(xr, zero),
               "moments F": lambda: K.feat_moments(xf, zero)}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in fns}
        for _ in range(opt.rounds):
            for name, fn in fns.items():          # the kernel and the ATen composition alternate inside every round
                times[name].append(timed(fn))
        got, ref = fns["scan F|R (radii)"](), fns["ATen  F|R (radii)"]()
        agree = float((got[1][:, 0] == ref[1][:, 0]).float().mean())
        flop = 2.0 * n * n * opt.dim
        lines.append(f"N = M = {n}")
        for name, v in times.items():
            best = min(v)
            rate = f"   {flop / best / 1e9:7.1f} TFLOP/s = {100 * flop / best / 1e9 / PEAK_F32_MFMA_TFLOPS:5.1f} % of the fp32 MFMA peak" \
                if "scan" in name or "ATen" in name else ""
            lines.append(f"  {name:26s}" + "  ".join(f"{x:10.3f}" for x in v) + f"   min {best:10.3f} ms{rate}")
        scans = sum(min(times[name]) for name in times if name.startswith("scan"))
        moms = min(times["moments R"]) + min(times["moments F"])
        ratio = min(times["scan F|R (radii)"]) / min(times["ATen  F|R (radii)"])
        lines += [f"  four scans {scans:.1f} ms + two moment passes {moms:.1f} ms = {scans + moms:.1f} ms per metric evaluation",
                  f"  dvq_pair_scan / ATen composition on F|R: {ratio:.2f} x ({'faster' if ratio < 1 else 'SLOWER'}); nearest neighbour agrees on "
                  f"{100 * agree:.2f} % of rows; the ATen form holds an N x {opt.chunk} block and is not reproducible across chunk sizes", ""]
        del xr, xf, ws
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
