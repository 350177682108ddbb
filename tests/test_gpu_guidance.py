"""Classifier-free guidance on the GPU (docs/design/14-guidance.md): the guided draw kernel dvq_sample_guided against
dvq_sample_constrained and an fp64 restatement, dvq_label_dropout, label dropout in training, and guided sampling through the whole
sampler, its concurrent lanes and the class-conditional sampling script."""
import os

import numpy as np
import pytest
import torch

from test_gpu_stage2 import _torch_draw_probs, dualformer_config

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLASSES = 10


def class_config(null_rows=True, cond_drop_prob=0.0, pdrop=0.0):
    """the small class-conditional Dualformer of test_gpu_stage2, every table one row larger (the null label) when null_rows"""
    cfg = dualformer_config()
    p = cfg["params"]
    extra = 1 if null_rows else 0
    p["transformer_config"]["params"].update(vocab_size=524 + extra, coarse_position_size=28 + extra, fine_position_size=76 + extra,
                                             embd_pdrop=pdrop, resid_pdrop=pdrop, attn_pdrop=pdrop)
    p["class_cond_stage_config"] = {"target": "modules.dynamic_modules.label_provider.ClassAwareSOSProvider", "params": dict(
        n_classes=N_CLASSES, threshold_content=514, threshold_coarse_position=18, threshold_fine_position=66, coarse_seg_sos=0,
        fine_seg_sos=1)}
    del p["uncond_stage_config"]
    if cond_drop_prob:
        p["cond_drop_prob"] = cond_drop_prob
    cfg["target"] = "models.stage2_dynamic.dqtransformer_class2_entropy.Dualformer"
    return cfg


def _rules_model():
    from dynamicvectorquantization_amd.stage2 import _SamplerMixinBase
    df = _SamplerMixinBase.__new__(_SamplerMixinBase)
    df.__dict__.update(coarse_position_pad_code=256, coarse_position_eos_code=257, max_coarse_postion_idx=255, fine_position_pad_code=1024,
                       fine_position_eos_code=1025, fine_position_sos_code=1026, content_pad_code=1024, content_eos_code=1025,
                       content_sos_code=1026)
    return df


def _cases(dev, b, g):
    """(kind, V, forbid lists of the 2B rows (pair halves identical) or None) for the three rules"""
    def twice(t):
        return torch.cat([t, t]).to(dev)
    return [("coarse_pos", 259, twice(torch.randint(0, 259, (b, 40), generator=g))),
            ("fine_pos", 1027, twice(torch.randint(0, 1027, (b, 300), generator=g))),
            ("content", 1027, None)]


def _done(dev, b):
    done = torch.zeros(2 * b, 1, device=dev)
    for r in (3, 11):
        done[r] = done[r + b] = 1
    return done


def _kernel_call(df, fn, logits, kind, sampled, done, state, sample, k, p, temperature=1.0, **extra):
    from dynamicvectorquantization_amd import kernels as K
    kw = df._fused_rule(kind)
    if kind != "content":
        kw["forbid_idx"] = sampled
    return getattr(K, fn)(logits, *extra.values(), temperature, state=state, finished=done, top_k=k, top_p=p, sample=sample, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guided_kernel_scale_one_is_conditional_and_zero_is_unconditional(dev, dtype):
    """s = 1: dvq_sample_guided == dvq_sample_constrained on the conditional rows, bit for bit, greedy and multinomial from the same
    generator state, for the three rules and top-k / top-p settings, dense and strided logits; the token sits in both halves.
    s = 0: greedy == dvq_sample_constrained on the unconditional rows (with the conditional rows' constraints)."""
    df = _rules_model()
    g = torch.Generator(device="cpu").manual_seed(11)
    b = 16
    done = _done(dev, b)
    for kind, v, sampled in _cases(dev, b, g):
        wide = (torch.randn(2 * b, v + 13, generator=g) * 3).to(dev).to(dtype)
        for logits in (wide[:, :v].contiguous(), wide[:, :v]):                    # dense, then a strided column slice
            fi_c = None if sampled is None else sampled[:b]
            for sample in (False, True):
                for k, p in [(None, None), (50, None), (None, 0.9), (20, 0.95)]:
                    st_a = torch.tensor([1234, 7], dtype=torch.int64, device=dev)
                    st_b = st_a.clone()
                    ref = _kernel_call(df, "sample_constrained", logits[:b], kind, fi_c, done[:b], st_a, sample, k, p)
                    got = _kernel_call(df, "sample_guided", logits, kind, sampled, done, st_b, sample, k, p, guidance=1.0)
                    assert got.shape == (2 * b, 1)
                    assert torch.equal(got[:b], ref), (kind, sample, k, p, logits.stride())
                    assert torch.equal(got[b:], got[:b])
                    assert torch.equal(st_a, st_b)
                ref0 = _kernel_call(df, "sample_constrained", logits[b:], kind, fi_c, done[:b], None, False, 50, None)
                got0 = _kernel_call(df, "sample_guided", logits, kind, sampled, done, None, False, 50, None, guidance=0.0)
                assert torch.equal(got0[:b], ref0) and torch.equal(got0[b:], ref0), kind


def test_guided_kernel_vs_fp64(dev):
    """s in {1.5, 4}: greedy == argmax of an fp64 restatement (rows with a top-2 gap below 1e-4 excluded, >= 90 % compared);
    4000 multinomial draws stay in the filtered support with total-variation distance < 0.06; one counter tick per call;
    finished rows always draw the pad code"""
    df = _rules_model()
    g = torch.Generator(device="cpu").manual_seed(5)
    b = 16
    done = _done(dev, b)
    pads = {"coarse_pos": 256, "fine_pos": 1024, "content": 1024}
    for s in (1.5, 4.0):
        for kind, v, sampled in _cases(dev, b, g):
            for dtype in (torch.float32, torch.bfloat16):
                logits = (torch.randn(2 * b, v, generator=g) * 2).to(dev).to(dtype)
                c64, u64 = logits[:b].double(), logits[b:].double()
                g64 = (1.0 - s) * u64 + s * c64
                rule = (kind, None if sampled is None else sampled[:b], done[:b])
                masked = torch.log(_torch_draw_probs(df, g64 / 0.8, 1.0, None, None, rule))     # masked logits - logsumexp
                top2 = masked.topk(2, dim=-1).values
                ok = (top2[:, 0] - top2[:, 1]) >= 1e-4
                assert int(ok.sum()) >= 0.9 * b, (kind, s)
                got = _kernel_call(df, "sample_guided", logits, kind, sampled, done, None, False, None, None, 0.8, guidance=s).view(-1)
                assert torch.equal(got[:b][ok], masked.argmax(dim=-1)[ok]), (kind, s, dtype)
                assert torch.equal(got[b:], got[:b])
            # multinomial (fp32 logits): support, frequencies, counter, finished rows
            ref = _torch_draw_probs(df, g64.float(), 1.0, 20, 0.95, rule)
            st = torch.tensor([99, 0], dtype=torch.int64, device=dev)
            n_draws = 4000
            counts = torch.zeros(2 * b, v, device=dev)
            for _ in range(n_draws):
                ix = _kernel_call(df, "sample_guided", logits.float(), kind, sampled, done, st, True, 20, 0.95, guidance=s)
                counts.scatter_add_(1, ix, torch.ones(2 * b, 1, device=dev))
            assert int(st[1]) == n_draws                                              # one tick per call
            assert torch.equal(counts[:b], counts[b:])                                # every draw in both halves
            assert float(counts[:b][ref == 0].sum()) == 0.0, (kind, s)                # never outside the filtered support
            tv = 0.5 * (counts[:b] / n_draws - ref).abs().sum(dim=1)
            assert float(tv.max()) < 0.06, (kind, s, tv)
            assert float(counts[3, pads[kind]]) == n_draws and float(counts[11, pads[kind]]) == n_draws


def test_guided_kernel_rejects_bad_guidance(dev):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import DvqError
    lg = torch.zeros(4, 64, device=dev)
    for s in (float("nan"), float("inf")):
        with pytest.raises(DvqError):
            K.sample_guided(lg, s, 1.0, pad_code=0, state=None, sample=False)


def test_label_dropout(dev):
    """p = 0: identity; p = 1: all null; p = 0.1 over 2^20 labels: drop rate within 5 sigma, and the dropped set is exactly the set
    dvq_dropout zeroes for the same seed; same seed -> same output, another seed -> another"""
    from dynamicvectorquantization_amd import kernels as K
    n = 1 << 20
    lab = torch.randint(0, 1000, (n,), device=dev)
    assert torch.equal(K.label_dropout(lab, 0.0, 1000, 17), lab)
    assert bool((K.label_dropout(lab, 1.0, 1000, 17) == 1000).all())
    a = K.label_dropout(lab, 0.1, 1000, 17)
    rate = float((a == 1000).double().mean())
    assert abs(rate - 0.1) < 5 * (0.1 * 0.9 / n) ** 0.5, rate
    assert torch.equal(a[a != 1000], lab[a != 1000])
    dropped = K.dropout(torch.ones(n, device=dev), 0.1, 17) == 0
    assert torch.equal(a == 1000, dropped)
    assert torch.equal(K.label_dropout(lab, 0.1, 1000, 17), a)
    assert not torch.equal(K.label_dropout(lab, 0.1, 1000, 18), a)
    small = torch.tensor([[1], [2], [3]], device=dev, dtype=torch.int32)
    assert K.label_dropout(small, 0.0, 10, 1).view(-1).tolist() == [1, 2, 3]


def _spy_labels(model, seen):
    orig = model.encode_to_c

    def spy(c):
        seen.append(c.detach().clone())
        return orig(c)
    model.encode_to_c = spy


def test_training_label_dropout(dev):
    """cond_drop_prob = 1 trains on the null label: one fp32 step (no other dropout) feeds the transformer the same start tokens as
    cond_drop_prob = 0 given null labels, and gives the same losses (to fp32 summation order: the loss sums are atomic);
    eval / validation never drop; without null rows construction and guided_conditioning raise before any launch"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.trainer import Trainer
    x = torch.from_numpy(synth.half_flat_images(3, 64, seed=5)).to(dev)
    lab = torch.tensor([1, 4, 9], device=dev)
    runs = {}
    with rt.compute_dtype_ctx(torch.float32):
        for name, pdrop, labels in (("drop", 1.0, lab), ("null", 0.0, torch.full_like(lab, N_CLASSES))):
            torch.manual_seed(2)
            model = instantiate_from_config(class_config(cond_drop_prob=pdrop)).to(dev)
            model.learning_rate, model.min_learning_rate, model.training_steps, model.steps_per_epoch = 1e-3, 0.0, 100, 10
            model.train()
            seen = []
            _spy_labels(model, seen)
            losses = Trainer(model, max_steps=1, use_graph=False).train_step({"image": x, "class_label": labels}, 0)
            runs[name] = ([float(l) for l in losses], seen[0], dict(model._logged))
            if name == "drop":
                model.validation_step({"image": x, "class_label": lab}, 0)          # train mode, validation: no drop
                assert torch.equal(seen[-1], lab)
                model.eval()
                model(x, lab)                                                       # eval forward: no drop
                assert torch.equal(seen[-1], lab)
    assert torch.equal(runs["drop"][1], runs["null"][1]) and bool((runs["drop"][1] == N_CLASSES).all())
    for a, b_ in zip(runs["drop"][0], runs["null"][0]):
        assert np.isfinite(a) and abs(a - b_) <= 1e-6 * abs(b_), runs
    for key in runs["null"][2]:
        a, b_ = float(runs["drop"][2][key]), float(runs["null"][2][key])
        assert abs(a - b_) <= 1e-6 * max(abs(b_), 1e-30), key
    # no null rows
    with pytest.raises(ValueError, match="vocab_size"):
        instantiate_from_config(class_config(null_rows=False, cond_drop_prob=0.1))
    model = instantiate_from_config(class_config(null_rows=False)).to(dev).eval()
    calls = []
    _lib._launch_hook = calls.append
    try:
        with pytest.raises(ValueError, match="null-label row"):
            model.guided_conditioning(lab)
    finally:
        _lib._launch_hook = None
    assert calls == []


def _guided_model(dev, seed=3):
    from dynamicvectorquantization_amd.config import instantiate_from_config
    torch.manual_seed(seed)
    model = instantiate_from_config(class_config()).to(dev).eval()
    with torch.no_grad():
        for n_, p_ in model.transformer.named_parameters():
            if n_.endswith("head.1.weight"):
                p_.mul_(6.0)                     # spread logits: greedy picks far from ties
    return model


KEYS4 = ("coarse_content", "fine_content", "coarse_position", "fine_position")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kv_cache", [True, False])
def test_guided_sampler_limits(dev, dtype, kv_cache):
    """whole sampler, greedy: guided s = 1 on [labels ; null] == plain sampling of [labels ; labels] (first B rows), s = 0 == plain
    sampling of [null ; null], token for token -- both halves carry identical inputs, so the batch composition is the same.
    s = 0 is compared with fixed fine positions only: a guided pair draws under its CONDITIONAL row's rules, and the class model's
    fine-position rule forbids the row's own start token, threshold_coarse_position + label, which is also a fine-position id
    (the reference's rule) -- so with drawn fine positions s = 0 differs from null sampling by exactly that one forbidden id."""
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(dtype):
        model = _guided_model(dev)
        lab = torch.tensor([1, 4, 9], device=dev)
        null = torch.full_like(lab, N_CLASSES)
        b = lab.numel()
        for fix in (False, True):
            kw = dict(sample=False, top_k=20, top_k_pos=10, process=False, fix_fine_position=fix, kv_cache=kv_cache)
            gc = model.guided_conditioning(lab)
            for s, plain_labels in ((1.0, torch.cat([lab, lab])), (0.0, torch.cat([null, null]))):
                if s == 0.0 and not fix:
                    continue
                got = model.sample_from_scratch(*gc, cfg_scale=s, **kw)
                ref = model.sample_from_scratch(*model.encode_to_c(plain_labels), **kw)
                for name, a, r in zip(KEYS4, got, ref):
                    assert a.shape[0] == b and torch.equal(a, r[:b]), (fix, s, name)
            g2 = model.sample_from_scratch(*gc, cfg_scale=3.0, **kw)
            assert int(g2[0].max()) <= 513 and int(g2[1].max()) <= 513 and int(g2[2].max()) <= 17 and int(g2[3].max()) <= 65
        with pytest.raises(ValueError, match="odd"):
            model.sample_from_scratch(*model.encode_to_c(lab), cfg_scale=2.0, **kw)


def test_guided_sample_many_lanes_equal_sequential(dev):
    """guided sample_many on 2 and 4 lanes == sequential guided sampling, greedy, batch by batch"""
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(torch.bfloat16):
        model = _guided_model(dev)
        labels = [torch.tensor(l, device=dev) for l in ([1, 4, 9], [0, 2, 3], [5, 5, 8], [7, 6, 1], [9, 0, 4])]
        conds = [model.guided_conditioning(l) for l in labels]
        kw = dict(sample=False, top_k=20, top_k_pos=10, process=False, fix_fine_position=False, cfg_scale=2.0)
        seq = [[t.cpu() for t in model.sample_from_scratch(*c, **kw)] for c in conds]
        assert all(t.shape[0] == 3 for t in seq[0])
        for lanes in (2, 4):
            got = model.sample_many(conds, n_streams=lanes, **kw)
            for i, (a, b_) in enumerate(zip(seq, got)):
                assert all(torch.equal(x_, y_.cpu()) for x_, y_ in zip(a, b_)), (lanes, i)


def _write_yaml(path, cfg):
    import yaml

    def plain(o):
        if isinstance(o, dict):
            return {k: plain(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        return o
    with open(path, "w", encoding="utf-8") as f:
        yaml.safe_dump({"model": plain(cfg)}, f)


def test_class_sampling_script_end_to_end(dev, tmp_path):
    """scripts/sample_val/sample_dynamic_class.py on the small model: --cfg_scale 2 --classes 0,3,7 --per_class 2 --npz writes the
    npz (uint8 NHWC, labels in class order) and the pickles; --cfg_scale 1 runs on tables without a null row"""
    import subprocess
    import sys
    script = os.path.join(REPO, "scripts/sample_val/sample_dynamic_class.py")
    for name, null_rows, extra in (("cfg", True, ["--cfg_scale", "2", "--npz"]), ("plain", False, ["--cfg_scale", "1"])):
        y = tmp_path / f"{name}.yml"
        _write_yaml(str(y), class_config(null_rows=null_rows))
        out = tmp_path / name
        r = subprocess.run([sys.executable, script, "--yaml_path", str(y), "--classes", "0,3,7", "--per_class", "2", "--batch_size", "4",
                            "--top_k", "20", "--top_k_pos", "10", "--seed", "3", "--out_dir", str(out)] + extra,
                           capture_output=True, text=True, timeout=900, cwd=REPO)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "images/s" in r.stdout
        tag = "TopK-20-10_TopP-1.0-1.0_Temp-1.0_CFG-{}".format(2.0 if name == "cfg" else 1.0)
        assert sorted(os.listdir(str(out / (tag + "_pickle")))) == ["samples_(0_2).pkl", "samples_(1_2).pkl"]
        if name == "cfg":
            f = np.load(str(out / (tag + "_npz") / "samples_6x64x64x3.npz"))
            assert f["arr_0"].dtype == np.uint8 and f["arr_0"].shape == (6, 64, 64, 3) and int(f["arr_0"].max()) > 0
            assert f["arr_1"].dtype == np.int64 and f["arr_1"].tolist() == [0, 0, 3, 3, 7, 7]
        else:
            assert not os.path.exists(str(out / (tag + "_npz")))
