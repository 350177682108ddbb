"""Host restatement of an optimizer step over an accumulation window (docs/design/28-gradient-accumulation.md): the gradients of a
window's micro-batches, each scaled by fl(1 / k), are added in fp32 in arrival order; Adam / AdamW (torch.optim's update, no amsgrad,
decoupled decay) is applied once, to the sum.  numpy only."""
import numpy as np


def accumulate(micro_grads, k):
    """fp32 sum of g_i * fl(1 / k) in arrival order; a short window (fewer than k micro-batches) is still divided by k"""
    inv = np.float32(1.0 / k)
    acc = np.zeros_like(micro_grads[0], dtype=np.float32)
    for g in micro_grads:
        acc += g.astype(np.float32) * inv
    return acc


class AdamOverWindows:
    """one parameter tensor; step(window) applies one update with the window's accumulated gradient"""

    def __init__(self, p, lr, betas, eps=1e-8, weight_decay=0.0):
        self.p = p.astype(np.float64).copy()
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.lr, self.betas, self.eps, self.wd, self.t = lr, betas, eps, weight_decay, 0

    def step(self, micro_grads, k):
        g = accumulate(micro_grads, k).astype(np.float64)
        b1, b2 = self.betas
        self.t += 1
        self.p *= 1.0 - self.lr * self.wd
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        self.p -= (self.lr / bc1) * self.m / (np.sqrt(self.v) / np.sqrt(bc2) + self.eps)
        return g


# ---- the reference's two-optimizer schedule over accumulation windows -------------------------------------------------------------------
ACCUM = dict(k=2, micro_batches=6, batches_per_epoch=4, warmup_steps=1, max_steps=50)      # three windows; window 0 at lr 0, window 2 opens epoch 1


def accum_stride(n):
    """an eighth of the samples the one-step fixtures keep per watched tensor: three windows of gradients fit the file"""
    from golden_cfg import train_step_stride
    return 8 * train_step_stride(n)


def run_window_steps(state, param_keys, batches, threshold, k, batches_per_epoch, lr, min_lr, warmup_steps, max_steps, restart_perm,
                     watch, stride):
    """oracle.train_step.run_steps with Lightning 1.5's accumulation around it: per micro-batch b and optimizer i -- gradients zeroed on
    a window's first micro-batch only, (loss / k).backward(), and on the closing micro-batch Adam and the scheduler.  Keys: run_steps'
    per micro-batch (s<b>.o<i>.{loss,codes,gap,cluster_size_ema,embed_ema,codebook}, s<b>.log.*); on closing micro-batches also
    s<b>.o<i>.lr, s<b>.grad.<name> (the accumulated gradient in front of Adam) and s<b>.{param,exp_avg,exp_avg_sq}.<name>."""
    import torch
    from dynamicvectorquantization_amd.trainer import window_flags
    from oracle import entropy as oent
    from oracle import losses as olo
    from oracle import train_step as ots
    CB = ots.CB
    sd, sd_d, sd_l = ots._split_state(state)
    pk = set(str(n) for n in param_keys)
    ae_named = {n: state[n] for n in state if n in pk and not n.startswith("loss.")}
    d_named = {n: state[n] for n in state if n in pk and n.startswith("loss.discriminator.")}
    opt_ae, opt_d = ots.Adam(ae_named, lr, (0.5, 0.9)), ots.Adam(d_named, lr, (0.5, 0.9))
    mult_min = (min_lr / lr) if lr else 0.0
    out, sched_t, pos = {}, 0, 0

    def sample(a):
        a = np.asarray(a).reshape(-1)
        return a[:: stride(a.size)].astype(np.float32).copy()

    def snap(pre):
        kk = sd[CB + "embed_ema"].shape[0]
        out[pre + "cluster_size_ema"] = sd[CB + "cluster_size_ema"].numpy().copy()
        out[pre + "embed_ema"] = sd[CB + "embed_ema"].numpy()[:: max(1, kk // 32)].copy()
        out[pre + "codebook"] = sd[CB + "weight"].detach().numpy()[:-1][:: max(1, kk // 32)].copy()

    def toggle(named, on, zero):
        for n, v in named.items():
            v.requires_grad_(on and n != CB + "weight")
            if zero:
                v.grad = None

    for v in list(ae_named.values()) + list(d_named.values()):
        v.requires_grad_(False)
        v.grad = None
    for b, x in enumerate(batches):
        x = torch.as_tensor(x)
        first, last = window_flags(pos, b % batches_per_epoch if batches_per_epoch else b, k, batches_per_epoch)
        cur_lr = lr * ots.lr_multiplier("linear-warmup_cosine-decay", warmup_steps, max_steps, mult_min, sched_t)
        lg = f"s{b}.log."
        # ---- optimizer 0 ----
        toggle(ae_named, True, first)
        toggle(d_named, False, False)
        info, run = {}, {}
        rec, qloss = ots.ae_forward(sd, x, threshold, restart_perm=restart_perm[b], record=info)
        r = olo.generator_loss(sd_d, sd_l, x, rec, qloss, sd["decoder.conv_out.weight"], running=run)
        (r["loss"] / k).backward()
        ots._bn_commit(sd_d, run, 1)
        pre = f"s{b}.o0."
        if last:
            for n in watch:
                if n in ae_named and ae_named[n].grad is not None:
                    out[f"s{b}.grad.{n}"] = sample(ae_named[n].grad.numpy())
            opt_ae.step(cur_lr)
            out[pre + "lr"] = np.float64(cur_lr)
        out[pre + "loss"] = np.float32(r["loss"].item())
        out[pre + "codes"], out[pre + "gap"] = info["codes"].astype(np.int16), info["gap"].astype(np.float32)
        snap(pre)
        for name, val in (("train_aeloss", r["loss"]), ("train_total_loss", r["loss"]), ("train_quant_loss", qloss), ("train_nll_loss", r["nll"]),
                          ("train_rec_loss", r["rec_mean"]), ("train_p_loss", r["p"].mean()), ("train_d_weight", r["d_weight"]), ("train_g_loss", r["g"])):
            out[lg + name] = np.float32(val.item())
        out[lg + "train_disc_factor"] = np.float32(1.0)
        out[lg + "train_fine_ratio"] = np.float32(oent.entropy_gate(oent.patch_entropy(x.numpy()), threshold)[..., 1].mean())
        # ---- optimizer 1 ----
        toggle(ae_named, False, False)
        toggle(d_named, True, first)
        info, run = {}, {}
        with torch.no_grad():
            rec2, _ = ots.ae_forward(sd, x, threshold, restart_perm=restart_perm[b], record=info)
        d_loss, lr_, lf_ = olo.discriminator_loss(sd_d, x, rec2, running=run)
        (d_loss / k).backward()
        ots._bn_commit(sd_d, run, 2)
        pre = f"s{b}.o1."
        if last:
            for n in watch:
                if n in d_named and d_named[n].grad is not None:
                    out[f"s{b}.grad.{n}"] = sample(d_named[n].grad.numpy())
            opt_d.step(cur_lr)
            out[pre + "lr"] = np.float64(cur_lr)
        out[pre + "loss"] = np.float32(d_loss.item())
        out[pre + "codes"], out[pre + "gap"] = info["codes"].astype(np.int16), info["gap"].astype(np.float32)
        snap(pre)
        out[lg + "train_discloss"] = out[lg + "train_disc_loss"] = np.float32(d_loss.item())
        out[lg + "train_logits_real"], out[lg + "train_logits_fake"] = np.float32(lr_.mean().item()), np.float32(lf_.mean().item())
        if last:
            sched_t += 1
            for n in watch:
                opt = opt_d if n in d_named else opt_ae
                out[f"s{b}.param.{n}"] = sample(state[n].detach().numpy())
                out[f"s{b}.exp_avg.{n}"] = sample(opt.state[n]["m"])
                out[f"s{b}.exp_avg_sq.{n}"] = sample(opt.state[n]["v"])
        pos = 0 if last else pos + 1
    toggle(ae_named, False, False)
    toggle(d_named, False, False)
    for n, v in sd_d.items():
        if n not in {m[len("loss.discriminator."):] for m in d_named}:
            out["final.disc_buf." + n] = v.numpy().copy()
    return out


def accum_schedule_steps(meta):
    """the pinned windowed run (ACCUM) of the `small` model from its deterministic start state; meta = the fixture's state_keys /
    state_shapes / param_keys"""
    import os
    from dynamicvectorquantization_amd import synth
    from golden_cfg import TRAIN_STEP, TRAIN_STEP_WATCH
    from oracle import entropy as oent
    from oracle import train_step as ots
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c, a = TRAIN_STEP["small"], ACCUM
    g = synth.DQVAE_GEOM[c["geom"]]
    state = ots.pinned_start_state(meta, g["k"], g["zc"])
    thr = oent.threshold_from_table(os.path.join(here, "scripts/tools/thresholds/entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
    perms = [synth.train_step_restart_perm(b, c["bs"], g["k"], g["resolution"]) for b in range(a["micro_batches"])]
    return run_window_steps(state, [str(n) for n in meta["param_keys"]], synth.train_step_batches(a["micro_batches"], c["bs"], g["resolution"]),
                            thr, a["k"], a["batches_per_epoch"], c["lr"], c["min_lr"], a["warmup_steps"], a["max_steps"], perms,
                            TRAIN_STEP_WATCH, accum_stride)
