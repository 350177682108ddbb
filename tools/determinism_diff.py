#!/usr/bin/env python3
"""Find the first tensor that differs between two runs of the same seeded training steps (docs/design/21-reproducible-training.md).

The same model is built twice in ONE process from the same seed and trained on the same batches under Trainer(deterministic=True)
(`--no-deterministic`: the default kernels, to see what the mode removes).  In every step, at every phase -- the gradients each
optimizer is about to apply (`o<i>.grad`) and the state after the step (`end`) -- every gradient, parameter, Adam moment, buffer (EMA
/ codebook / BatchNorm statistics) and logged scalar is hashed on the host (SHA-1 of the bytes).  The second run is compared with
the first as it goes; the first differing tensor is printed with its step and phase, then how many tensors differed at each later
phase.  Hashes only: nothing is printed from the device.

    python tools/determinism_diff.py --stage 1 --geom small --dtype bf16 --steps 10
    python tools/determinism_diff.py --stage 2 --dtype bf16 --steps 10

Stage 1: the shrunken DQ-VAEs of the tests (`--geom small | c1`: tests/test_gpu_model.GEOM, complete objective with the
discriminator).  Stage 2: the Dualformer of tests/golden_cfg.dualformer_cfg on the frozen small DQ-VAE (`--pdrop` sets its three
dropout rates).  Exit status 1 if anything differed (or if a deterministic run counted an unordered launch)."""
import argparse
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", type=int, default=1, choices=[1, 2])
    ap.add_argument("--geom", default="small", help="stage 1: small | c1")
    ap.add_argument("--dtype", default="bf16", help="bf16 | fp32 | fp32x3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=0, help="0: the pinned run's batch size")
    ap.add_argument("--pdrop", type=float, default=-1.0, help="stage 2: dropout rates (default: the config's)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-deterministic", dest="deterministic", action="store_false")
    opt = ap.parse_args()
    import numpy as np
    import torch

    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.trainer import Trainer
    dev = torch.device("cuda:0")

    def digest(t):
        return hashlib.sha1(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

    def build():
        torch.manual_seed(opt.seed)
        if opt.stage == 1:
            from golden_cfg import TRAIN_STEP
            from test_gpu_model import GEOM, model_config
            c = TRAIN_STEP[opt.geom]
            g = GEOM[c["geom"]]
            model = instantiate_from_config(model_config(**g, loss="full", ndf=c["ndf"])).to(dev)
            synth.apply_train_step_state(model, g["k"], g["zc"])
            model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
            model.warmup_epochs, model.steps_per_epoch, model.training_steps = c["warmup_epochs"], c["steps_per_epoch"], max(c["training_steps"], opt.steps)
            bs = opt.batch or c["bs"]
            batches = [torch.from_numpy(xb).to(dev) for xb in synth.train_step_batches(opt.steps, bs, g["resolution"])]
        else:
            from conftest import load_golden
            from golden_cfg import TRAIN_STEP_S2, dualformer_cfg, train_step_s2_batch
            from test_oracle_golden import dqvae_state_dict
            c = TRAIN_STEP_S2
            cfg = dualformer_cfg("uncond", os.path.join(REPO, "scripts/tools/thresholds/entropy_thresholds_imagenet_train_patch-16.json"))
            cfg["weight_decay"], cfg["warmup_epochs"] = c["weight_decay"], c["warmup_epochs"]
            if opt.pdrop >= 0:
                for k_ in ("embd_pdrop", "resid_pdrop", "attn_pdrop"):
                    cfg["transformer_config"]["params"][k_] = opt.pdrop
            model = instantiate_from_config({"target": "models.stage2_dynamic.dqtransformer_uncond_entropy.Dualformer", "params": cfg}).to(dev)
            model.first_stage_model.load_state_dict(dqvae_state_dict(load_golden("dqvae_small"), "spread", 512, 64))
            with torch.no_grad():
                for n, p in model.transformer.named_parameters():
                    p.copy_(torch.from_numpy(synth.det_param("dualformer.uncond." + n, tuple(p.shape)) * (0.3 if n == "pos_emb" else 1.0)).to(dev))
            model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
            model.steps_per_epoch, model.training_steps = c["steps_per_epoch"], max(c["training_steps"], opt.steps)
            batches = [torch.from_numpy(train_step_s2_batch(s % 3)).to(dev) for s in range(opt.steps)]
        rt.bump_weights_epoch()
        model.train()
        return model, batches

    def run(on_phase):
        """on_phase(step, phase, {name: digest}) at every phase of every step"""
        model, batches = build()
        tr = Trainer(model, max_steps=opt.steps, use_graph=False, deterministic=opt.deterministic)
        if not opt.deterministic:
            K.set_deterministic(False)
            rt.reseed_draws(model)
        cur = {"step": 0}

        def state(grads_of=None):
            torch.cuda.synchronize()
            h = {}
            if grads_of is not None:
                for gi, grp in enumerate(grads_of.param_groups):
                    for pi, p in enumerate(grp["params"]):
                        if p.grad is not None:
                            h[f"grad.{names.get(id(p), f'g{gi}.p{pi}')}"] = digest(p.grad)
                return h
            for n, p in model.named_parameters():
                h["param." + n] = digest(p)
            for n, b in model.named_buffers():
                h["buffer." + n] = digest(b)
            for oi, o in enumerate(tr.opts):
                for key in ("m", "v"):
                    if key in getattr(o, "_fstate", {}):
                        h[f"adam.o{oi}.{'exp_avg' if key == 'm' else 'exp_avg_sq'}"] = digest(o._fstate[key])
            for k_, v_ in getattr(model, "_logged", {}).items():
                h["log." + k_] = digest(torch.as_tensor(v_).float())
            return h

        names = {id(p): n for n, p in model.named_parameters()}
        for oi, o in enumerate(tr.opts):
            def wrapped(closure=None, _o=o, _oi=oi, _orig=o.step):
                on_phase(cur["step"], f"o{_oi}.grad", state(_o))
                return _orig(closure)
            o.step = wrapped
        for step, xb in enumerate(batches):
            cur["step"] = step
            losses = tr.train_step({"image": xb}, step)
            h = state()
            for oi, l in enumerate(losses):
                h[f"loss.o{oi}"] = digest(l.float())
            on_phase(step, "end", h)

    first, record, report = {}, [], []

    def remember(step, phase, h):
        first[(step, phase)] = h
        record.append((step, phase))

    def compare(step, phase, h):
        ref = first.get((step, phase), {})
        bad = sorted(k for k in set(ref) | set(h) if ref.get(k) != h.get(k))
        report.append((step, phase, len(h), bad))

    try:
        K.set_deterministic(opt.deterministic)
        c0 = K.unordered_launches()
        with rt.compute_dtype_ctx(opt.dtype):
            run(remember)
            run(compare)
        unordered = K.unordered_launches() - c0
    finally:
        K.set_deterministic(False)
    what = f"stage {opt.stage}" + (f" ({opt.geom})" if opt.stage == 1 else "") + f", {opt.dtype}, {opt.steps} steps, deterministic {opt.deterministic}"
    print(f"[determinism_diff] {what}: {len(report)} phases, {sum(n for _, _, n, _ in report)} tensors hashed per run, "
          f"{unordered} unordered launches counted over both runs")
    differing = [r for r in report if r[3]]
    if not differing:
        print("[determinism_diff] no difference")
    else:
        step, phase, n, bad = differing[0]
        print(f"[determinism_diff] FIRST DIFFERENCE: step {step}, phase {phase}: {bad[0]}  ({len(bad)} of {n} tensors differ at this phase)")
        for b in bad[1:8]:
            print(f"[determinism_diff]     also {b}")
        for step, phase, n, bad in differing[1:12]:
            print(f"[determinism_diff]   step {step}, phase {phase}: {len(bad)} of {n} differ, first {bad[0]}")
    return 1 if differing or (opt.deterministic and unordered) else 0


if __name__ == "__main__":
    sys.exit(main())
