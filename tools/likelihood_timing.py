#!/usr/bin/env python3
"""Cost of the stage-2 likelihood evaluation next to the validation step it extends (docs/design/15-likelihood.md).

On the batches of configs/stage2/uncond_imagenet_p6c18.yml (its batch size, 256 x 256 synthetic images, random weights, bf16), timed
with HIP events after a warm-up, in alternating rounds: Dualformer.validation_step per batch against evaluate_likelihood over the same
batches; behind the codes, StackGPT's with-loss forward against StackGPT.score; and the kernels alone at the step's logits shape
(dvq_cross_entropy, dvq_token_nll, dvq_nll_segment_sums).  Writes the table to --out (and prints it).

    python tools/likelihood_timing.py --out profiles/likelihood_timing.txt
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0, help="0: the YAML's data.params.batch_size")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per kernel timing")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    import torch

    from dynamicvectorquantization_amd import config as cfg
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    dev = torch.device("cuda:0")
    rt.set_compute_dtype(opt.dtype)
    yml = os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml")
    bs = opt.batch or int(cfg.load_yaml(yml).data.params.batch_size)
    model, size = E.load_stage2_model(yml, "", dev)
    xs = [{"image": torch.from_numpy(synth.half_flat_images(bs, size, seed=300 + i)).to(dev)} for i in range(opt.batches)]

    def timed(fn, reps=1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    def val_loop():
        for i, b in enumerate(xs):
            model.validation_step(b, i)

    def like_loop():
        E.evaluate_likelihood(model, xs)

    with torch.no_grad():
        _, z = model.encode_to_z(xs[0]["image"])
        inp = model.teacher_forcing_inputs(z, model.encode_to_c(xs[0]["image"]))
        tr = model.transformer
        pl, cl, b, t, tp = tr.fwd(inp["coarse_content"], inp["fine_content"], inp["coarse_position"], inp["fine_position"],
                                  inp["coarse_seg"], inp["fine_seg"], None)
        tg = tr._targets(b, t, tp, inp["coarse_position"].shape[1], inp["content_target"], inp["coarse_position_target"],
                         inp["fine_position_target"], dev)
        vc = tr.config.vocab_size
        acc = torch.zeros(2, dtype=torch.float32, device=dev)
        nll, rank = K.token_nll(cl, vc, tg[0][0], tg[0][1])
        for _ in range(2):                                    # warm-up of every shape the timed windows use
            val_loop()
            like_loop()
            tr(**inp)
            tr.score(**inp)
        torch.cuda.synchronize()
        val, like, fwd, score = [], [], [], []
        for _ in range(opt.rounds):
            val.append(timed(val_loop) / opt.batches)
            like.append(timed(like_loop) / opt.batches)
            fwd.append(timed(lambda: tr(**inp), 5))
            score.append(timed(lambda: tr.score(**inp), 5))
        # host-side pieces of the scoring path that the validation step does not have (host clock; the second ends in a synchronise)
        import time
        def flags():
            on = [m for m in tr.modules() if m.training]
            for m in on:
                m.training = False
            for m in on:
                m.training = True

        t_flags = []
        for mode in (False, True):                            # evaluation finds the model in eval mode; a validation hook in train mode
            tr.train(mode)
            t0 = time.perf_counter()
            for _ in range(20):
                flags()
            t_flags.append((time.perf_counter() - t0) / 20 * 1e3)
        tr.eval()
        meter = E.LikelihoodMeter()
        for b_ in xs:
            meter.update(model.score(*model.get_xc(b_)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        meter.summary()
        t_summary = (time.perf_counter() - t0) * 1e3
        t_ce = timed(lambda: K.cross_entropy(cl, vc, tg[0][0], tg[0][1], acc[0:1], acc[1:2]), opt.reps)
        t_nll = timed(lambda: K.token_nll(cl, vc, tg[0][0], tg[0][1]), opt.reps)
        t_seg = timed(lambda: K.nll_segment_sums(nll, rank, b, tp, tp // 2), opt.reps)
    rows, ldl = cl.shape
    mb = rows * ldl * cl.element_size() / 1e6
    fmt = lambda v: "  ".join(f"{x:8.3f}" for x in v) + f"   min {min(v):8.3f} ms"
    lines = [
        f"likelihood-evaluation cost, uncond_imagenet_p6c18.yml, random weights, {opt.dtype}, batch {bs} x {size} x {size}, "
        f"{torch.cuda.get_device_name(0)} (tools/likelihood_timing.py; HIP events, after warm-up, {opt.rounds} alternating rounds)",
        "",
        f"per batch over {opt.batches} batches (frozen DQ-VAE encode + permuter + StackGPT; T = {t}, padded {tp}):",
        f"  Dualformer.validation_step          {fmt(val)}",
        f"  evaluate_likelihood (incl. summary) {fmt(like)}",
        f"  likelihood / validation (min over rounds): {min(like) / min(val):.3f}x",
        "",
        "behind the codes, one batch (5 calls per round):",
        f"  StackGPT with-loss forward          {fmt(fwd)}",
        f"  StackGPT.score                      {fmt(score)}",
        f"  score / forward (min over rounds): {min(score) / min(fwd):.3f}x",
        "",
        "host work of the scoring path that validation_step does not do (host clock):",
        f"  Dualformer.score's eval-mode switch over {len(list(tr.modules()))} modules, per batch: found in eval mode {t_flags[0]:.3f} ms, "
        f"in train mode {t_flags[1]:.3f} ms",
        f"  LikelihoodMeter.summary (cat, one copy to the host, numpy), once per evaluation   {t_summary:8.3f} ms "
        f"= {t_summary / opt.batches:.3f} ms per batch here",
        "",
        f"kernels alone on the content logits [{rows}, {ldl}] ({mb:.1f} MB, V = {vc}), {opt.reps} calls each:",
        f"  dvq_cross_entropy (loss only)       {t_ce * 1e3:9.1f} us   ({mb / t_ce:.0f} GB/s of logits read)",
        f"  dvq_token_nll                       {t_nll * 1e3:9.1f} us   ({mb / t_nll:.0f} GB/s of logits read)",
        f"  dvq_nll_segment_sums                {t_seg * 1e3:9.1f} us",
        "  (one step runs three of each: content, coarse position, fine position)",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        with open(opt.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
