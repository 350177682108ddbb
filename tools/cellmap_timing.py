#!/usr/bin/env python3
"""Cost of the two cell-map passes next to the forwards they ride on (docs/design/30-cell-maps.md).

configs/stage2/uncond_imagenet_p6c18.yml with random weights, 256 x 256 synthetic images, one process, HIP events after a warm-up:
the reconstruction cell pass (dvq_recon_cells) next to dvq_recon_metrics and the frozen DQ-VAE's ae_fwd on the same batch, and the
likelihood cell pass (three dvq_nll_cell_sums launches + the paired-position vector) next to StackGPT's forward, score and score_cells.
The bar is docs/design/13-evaluation.md's: a metric pass stays under 1 % of the forward it measures.  Writes the table to --out.

    python tools/cellmap_timing.py --out profiles/cellmap_timing.txt
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per kernel timing")
    ap.add_argument("--fwd_reps", type=int, default=3, help="calls per forward timing")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import torch

    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    dev = torch.device("cuda:0")
    rt.set_compute_dtype(opt.dtype)
    model, size = E.load_stage2_model(os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml"), "", dev)
    vae, tr = model.first_stage_model, model.transformer
    bs = opt.batch
    x = torch.from_numpy(synth.half_flat_images(bs, size, seed=300)).to(dev)

    def timed(fn, reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    with torch.no_grad():
        out = vae.ae_fwd(x, None)
        rec, grain = out["rec"], out["grain"]
        hg, wg = int(grain.shape[1]), int(grain.shape[2])
        ws_img = K.recon_metrics_workspace(bs, size, size, dev)
        ws_cell = K.recon_cells_workspace(bs, size, size, hg, wg, dev)
        _, z = model.encode_to_z(x)
        inp = model.teacher_forcing_inputs(z, model.encode_to_c(x))
        pl, cl, b, t, tp = tr.fwd(inp["coarse_content"], inp["fine_content"], inp["coarse_position"], inp["fine_position"],
                                  inp["coarse_seg"], inp["fine_seg"], None)
        lc = inp["coarse_position"].shape[1]
        tg = tr._targets(b, t, tp, lc, inp["content_target"], inp["coarse_position_target"], inp["fine_position_target"], dev)
        rows = [K.token_nll(cl, tr.config.vocab_size, tg[0][0], tg[0][1]), K.token_nll(pl, tr.config.fine_position_size, tg[1][0], tg[1][1]),
                K.token_nll(pl, tr.config.fine_position_size, tg[2][0], tg[2][1])]
        hw1, hw2 = model.hw1, model.hw2
        cells = torch.zeros(b, 4, hw1 * hw1, 4, dtype=torch.float64, device=dev)
        outside = torch.zeros(b, 4, 4, dtype=torch.float64, device=dev)

        def cell_pass():
            paired = torch.full((b, tp), -1, dtype=torch.long, device=dev)
            paired[:, :t] = torch.cat([inp["coarse_position"], inp["fine_position"]], dim=1)[:, 1:]
            K.nll_cell_sums(*rows[0], paired.view(-1), b, tp, lc - 1, hw1, hw2, (0, 1), cells, outside)
            K.nll_cell_sums(*rows[1], tg[1][0], b, tp, tp, hw1, hw2, (2, -1), cells, outside)
            K.nll_cell_sums(*rows[2], tg[2][0], b, tp, 0, hw1, hw2, (-1, 3), cells, outside)

        def seg_pass():
            K.nll_segment_sums(*rows[0], b, tp, lc - 1)
            K.nll_segment_sums(*rows[1], b, tp, tp)
            K.nll_segment_sums(*rows[2], b, tp, 0)

        fns = {"ae_fwd": (lambda: vae.ae_fwd(x, None), opt.fwd_reps),
               "dvq_recon_metrics": (lambda: K.recon_metrics(x, rec, True, ws_img), opt.reps),
               "dvq_recon_cells": (lambda: K.recon_cells(x, rec, hg, wg, True, ws_cell), opt.reps),
               "StackGPT.fwd": (lambda: tr.fwd(inp["coarse_content"], inp["fine_content"], inp["coarse_position"], inp["fine_position"],
                                               inp["coarse_seg"], inp["fine_seg"], None), opt.fwd_reps),
               "StackGPT.score": (lambda: tr.score(**inp), opt.fwd_reps),
               "StackGPT.score_cells": (lambda: tr.score_cells(**inp, hw1=hw1, hw2=hw2), opt.fwd_reps),
               "3 x dvq_nll_segment_sums": (seg_pass, opt.reps),
               "cell pass (3 x dvq_nll_cell_sums + pairing)": (cell_pass, opt.reps)}
        for fn, _ in fns.values():                            # warm-up of every shape the timed windows use
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(opt.rounds):
            for k, (fn, reps) in fns.items():
                times[k].append(timed(fn, reps))
    best = {k: min(v) for k, v in times.items()}
    fmt = lambda v: "  ".join(f"{x:9.4f}" for x in v) + f"   min {min(v):9.4f} ms"
    r1 = best["dvq_recon_cells"] / best["ae_fwd"]
    ck = "cell pass (3 x dvq_nll_cell_sums + pairing)"
    r2 = best[ck] / best["StackGPT.fwd"]
    lines = [f"cell-map cost, uncond_imagenet_p6c18.yml, random weights, {opt.dtype}, batch {bs} x {size} x {size}, grid {hg} x {wg}, "
             f"T = {t} (padded {tp}), {torch.cuda.get_device_name(0)} (tools/cellmap_timing.py; HIP events, after warm-up, {opt.rounds} rounds, "
             f"one process)", ""]
    lines += [f"  {k:46s}{fmt(v)}" for k, v in times.items()]
    lines += ["",
              f"reconstruction cell pass / ae_fwd:          {100 * r1:.3f} %   (bar: < 1 %; dvq_recon_metrics: "
              f"{100 * best['dvq_recon_metrics'] / best['ae_fwd']:.3f} %)   {'under' if r1 < 0.01 else 'OVER'} the bar",
              f"likelihood cell pass / StackGPT forward:    {100 * r2:.3f} %   (bar: < 1 %; the three segment sums: "
              f"{100 * best['3 x dvq_nll_segment_sums'] / best['StackGPT.fwd']:.3f} %)   {'under' if r2 < 0.01 else 'OVER'} the bar"]
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
