#!/usr/bin/env python3
"""Generate tests/golden/train_step_accum_small.npz: the REAL reference (build container only, imported read-only through
tools/gen_golden.py's stubs) driven by hand through Lightning 1.5's automatic optimization with accumulate_grad_batches = k
(docs/design/28-gradient-accumulation.md): per micro-batch, per optimizer i -- toggle_optimizer(i), zero_grad on a window's first
micro-batch only, training_step, (loss / k).backward(), and on the closing micro-batch optimizer.step(); schedulers and global_step
advance when a window closes.  The `small` model of train_step_small.npz, k = 2, three windows, four batches per epoch; window 0 at
lr 0, window 1 at the full rate, window 2 opens the second epoch.  The restart permutation is injected as run_reference_train_steps
does.  Before the file is written, tests/accum_math.py's host restatement is held to it with oracle.train_step.PIN_BOUNDS.

    python tools/gen_golden_accum.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

sys.path.insert(0, os.path.join(G.REPO, "tests"))


def run_reference_windows():
    import accum_math as A
    from golden_cfg import TRAIN_STEP, TRAIN_STEP_WATCH, train_step_lossconfig
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.trainer import window_flags
    from oracle import vq as ovq
    from utils.utils import instantiate_from_config
    c, a = TRAIN_STEP["small"], A.ACCUM
    g = synth.DQVAE_GEOM[c["geom"]]
    k, zc, kacc = g["k"], g["zc"], a["k"]
    torch.manual_seed(0)
    model = G.build_dqvae(**g)
    model.loss = instantiate_from_config(train_step_lossconfig(c["ndf"]))
    synth.apply_train_step_state(model, k, zc)
    model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
    # the schedules count optimizer steps: warm-up of one step (window 0 at lr 0), cosine over max_steps
    model.warmup_epochs, model.steps_per_epoch, model.training_steps = 1.0, a["warmup_steps"], a["max_steps"]
    model.current_epoch, model.global_step = 0, 0
    logged = {}
    model.log = lambda name, value, **kw: logged.__setitem__(name, float(value))
    model.log_dict = lambda d, **kw: logged.update({kk: float(v) for kk, v in d.items()})
    model.train()
    model.loss.perceptual_loss.eval()
    opts, scheds = model.configure_optimizers()
    n_rows = c["bs"] * g["latent"] ** 2
    assert n_rows >= k
    perm = [None]
    orig_randperm = torch.randperm
    torch.randperm = lambda m, device=None, **kw: G.t(perm[0].copy()) if m == n_rows else orig_randperm(m, **kw)
    out = {}
    params = dict(model.named_parameters())
    cbm = model.quantize.codebook
    vq_in = []
    hook = cbm.register_forward_hook(lambda m, inp, outp: vq_in.append((inp[0].detach().reshape(-1, zc).numpy().copy(), outp[1].reshape(-1).numpy().copy())))

    def sample(tn):
        arr = tn.detach().reshape(-1).numpy()
        return arr[:: A.accum_stride(arr.size)].astype(np.float32).copy()

    pos = 0
    try:
        for b, xb in enumerate(synth.train_step_batches(a["micro_batches"], c["bs"], g["resolution"])):
            batch = {"image": G.t(xb)}
            perm[0] = synth.train_step_restart_perm(b, c["bs"], k, g["resolution"])
            bpe = a["batches_per_epoch"]
            model.current_epoch = b // bpe
            first, last = window_flags(pos, b % bpe, kacc, bpe)
            for oi, opt in enumerate(opts):
                owned = {id(p) for grp in opt.param_groups for p in grp["params"]}
                saved = {n_: p.requires_grad for n_, p in params.items()}
                for n_, p in params.items():           # LightningModule.toggle_optimizer
                    if id(p) not in owned:
                        p.requires_grad_(False)
                w_before = cbm.weight.detach().numpy()[:-1].copy()
                if first:
                    opt.zero_grad()
                loss = model.training_step(batch, b, oi)
                (loss / kacc).backward()
                pre = f"s{b}.o{oi}."
                if last:
                    for n_ in TRAIN_STEP_WATCH:
                        if id(params[n_]) in owned and params[n_].grad is not None:
                            out[f"s{b}.grad.{n_}"] = sample(params[n_].grad)
                    out[pre + "lr"] = np.float64(opt.param_groups[0]["lr"])
                    opt.step()
                for n_, p in params.items():           # untoggle_optimizer
                    p.requires_grad_(saved[n_])
                out[pre + "loss"] = np.float32(loss.item())
                x_in, codes = vq_in.pop()
                assert not vq_in
                _, gap = ovq.argmin_exact(x_in, w_before, return_gap=True)
                out[pre + "codes"], out[pre + "gap"] = codes.astype(np.int16), gap.astype(np.float32)
                out[pre + "cluster_size_ema"] = cbm.cluster_size_ema.numpy().copy()
                out[pre + "embed_ema"] = cbm.embed_ema.numpy()[:: k // 32].copy()
                out[pre + "codebook"] = cbm.weight.detach().numpy()[:-1][:: k // 32].copy()
            for k_, v_ in logged.items():
                out[f"s{b}.log.{k_}"] = np.float32(v_)
            if last:
                for sc in scheds:
                    sc["scheduler"].step()
                model.global_step += 1
                for n_ in TRAIN_STEP_WATCH:
                    opt = opts[1] if n_.startswith("loss.discriminator.") else opts[0]
                    st = opt.state[params[n_]]
                    out[f"s{b}.param.{n_}"] = sample(params[n_])
                    out[f"s{b}.exp_avg.{n_}"] = sample(st["exp_avg"])
                    out[f"s{b}.exp_avg_sq.{n_}"] = sample(st["exp_avg_sq"])
                    assert int(st["step"]) == model.global_step
            pos = 0 if last else pos + 1
    finally:
        torch.randperm = orig_randperm
        hook.remove()
    for n_, bf in model.loss.discriminator.named_buffers():
        out["final.disc_buf." + n_] = bf.numpy().copy()
    sd = model.state_dict()
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array([",".join(map(str, sd[kk].shape)) for kk in sd.keys()])
    out["param_keys"] = np.array([n_ for n_, _ in model.named_parameters()])
    return out


def main():
    import accum_math as A
    from dynamicvectorquantization_amd import synth
    from oracle import train_step as ots
    torch.manual_seed(0)
    torch.set_num_threads(8)
    G.install_stubs()
    out = run_reference_windows()
    for b in range(A.ACCUM["micro_batches"]):
        lr = out.get(f"s{b}.o0.lr")
        print(f"  micro-batch {b}: aeloss {out[f's{b}.o0.loss']:.6f} discloss {out[f's{b}.o1.loss']:.6f} min gap "
              f"{min(out[f's{b}.o0.gap'].min(), out[f's{b}.o1.gap'].min()):.2e}" + (f"  closes a window at lr {lr:.3e}" if lr is not None else ""))
    meta = {kk: out[kk] for kk in ("state_keys", "state_shapes", "param_keys")}
    o = A.accum_schedule_steps(meta)
    missing = [kk for kk in out if kk not in o and not kk.startswith(("state_", "param_keys"))]
    assert not missing, missing
    g = synth.DQVAE_GEOM["small"]
    summ = ots.summarize(ots.compare_records(o, out, start_param=ots.sampled_start_param(meta, g["k"], g["zc"], A.accum_stride)))
    for (step, grp), err in sorted(summ.items()):
        if not grp.startswith("scalar:train_"):
            print(f"  pin accum.{step}.{grp:24s} err={err:.3e}")
    bad = ots.check_summary(summ)
    if bad:
        raise SystemExit(f"tests/accum_math.py does not match the reference: {bad}")
    path = os.path.join(G.GOLD, "train_step_accum_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
