"""GPU tests of the DQ-Transformer likelihood scoring (docs/design/15-likelihood.md): dvq_token_nll / dvq_nll_segment_sums against
fp64 on the stored logits, StackGPT.score / Dualformer.score against the stage-2 goldens and the model's own with-loss forward, and
scripts/tools/eval_likelihood.py end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu


# ---- fp64 reference on the stored logits ---------------------------------------------------------------------------------------------
def nll_rank_ref(x64, target, ignore_index):
    """x64 fp64 [rows, V] (CPU), target int64 [rows] -> (nll fp64 [rows], rank int64 [rows]) by include/dvq_hip.h's definitions"""
    rows, v = x64.shape
    nll = torch.zeros(rows, dtype=torch.float64)
    rank = torch.full((rows,), -1, dtype=torch.int64)
    live = target != ignore_index
    if live.any():
        xl, tl = x64[live], target[live]
        xt = xl.gather(1, tl[:, None])
        nll[live] = torch.logsumexp(xl, dim=1) - xt[:, 0]
        cols = torch.arange(v)[None, :]
        rank[live] = (xl > xt).sum(1) + ((xl == xt) & (cols < tl[:, None])).sum(1)
    return nll, rank


def make_rows(rows, v, ldl, dtype, dev, seed, all_ignored=False):
    """logits [rows, ldl] of `dtype` on the device (padding columns = +1e4: a read past V shows in every result), targets, ignore index.
    Rows 0 .. 5 (as far as `rows` reaches): target 0; target V-1; ignored; +-80 magnitudes; -inf in non-target columns (every second
    row of this kind: in ALL of them); ties with the target's value on both sides of it.  The rest: N(0, 3) logits, a fifth ignored."""
    g = torch.Generator().manual_seed(seed)
    ign = v // 3 if v >= 8 else -100                          # the project's ignore indices are pad codes INSIDE the vocabulary
    x = torch.randn(rows, v, generator=g) * 3.0
    tg = torch.randint(0, v, (rows,), generator=g)
    tg = torch.where(tg == ign, torch.full_like(tg, (ign + 1) % v if v > 1 else 0), tg)
    tg[torch.rand(rows, generator=g) < 0.2] = ign
    if rows == 1:
        tg[0] = 0 if dtype == torch.float32 else v - 1
    for r in range(min(rows, 6)):
        if rows == 1:
            break
        if r == 0:
            tg[r] = 0
        elif r == 1:
            tg[r] = v - 1
        elif r == 2:
            tg[r] = ign
        elif r == 3:
            x[r] = (torch.rand(v, generator=g) * 2 - 1) * 80.0
            tg[r] = v // 2
        elif r == 4:
            tg[r] = v // 2
            mask = torch.rand(v, generator=g) < 0.5
            if seed % 2:
                mask[:] = True
            mask[v // 2] = False
            x[r, mask] = -float("inf")
        elif r == 5 and v >= 3:
            t = v // 2
            tg[r] = t
            x[r, t - 1] = x[r, t + 1] = x[r, t]
            if v >= 5:
                x[r, 0] = x[r, v - 1] = x[r, t]
    if all_ignored:
        tg[:] = ign
    full = torch.full((rows, ldl), 1e4)
    full[:, :v] = x
    return full.to(dtype).to(dev).contiguous(), tg.to(dev), ign


def check_token_nll(dev, rows, v, ldl, dtype, seed, all_ignored=False):
    """-> (kernel's worst |nll - fp64|, torch's fp32 F.cross_entropy's worst |.| on the same inputs = the yardstick)"""
    from dynamicvectorquantization_amd import kernels as K
    logits, tg, ign = make_rows(rows, v, ldl, dtype, dev, seed, all_ignored)
    x64 = logits[:, :v].double().cpu()                        # bf16 -> fp64 is exact
    ref_nll, ref_rank = nll_rank_ref(x64, tg.cpu(), ign)
    nll, rank = K.token_nll(logits, v, tg, ign)
    yard = torch.nn.functional.cross_entropy(logits[:, :v].float(), tg, ignore_index=ign, reduction="none")
    assert nll.dtype == torch.float32 and rank.dtype == torch.int32 and nll.shape == (rows,) and rank.shape == (rows,)
    assert torch.equal(rank.cpu().long(), ref_rank), (rank.cpu().tolist()[:8], ref_rank.tolist()[:8])
    assert bool(torch.isfinite(nll).all())
    dead = (tg == ign).cpu()
    assert bool((nll.cpu()[dead] == 0).all()) and bool((rank.cpu()[dead] == -1).all())
    err = float((nll.cpu().double() - ref_nll).abs().max())
    yard_err = float((yard.cpu().double() - ref_nll).abs().max())
    bound = max(4.0 * yard_err, 1e-6)
    print(f"token_nll rows={rows} V={v} ldl={ldl} {dtype}: kernel {err:.3e}  torch fp32 {yard_err:.3e}  bound {bound:.3e}")
    assert err <= bound, (err, yard_err)
    return err, yard_err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pitch", ["vec", "odd"])
@pytest.mark.parametrize("v", [1, 63, 64, 65, 1026, 1027])
@pytest.mark.parametrize("rows", [1, 7, 130])
def test_token_nll_vs_fp64(dev, rows, v, pitch, dtype):
    """nll within 4x the error of torch's own fp32 F.cross_entropy on the same inputs (floor 1e-6; both sum ~V fp32 terms in different
    orders), rank exact.  pitch "vec": the row pitch is the next multiple of 8 above V (rows held in registers, 16-byte loads);
    "odd": V + 3 (the one-pass kernel).  Measured: docs/design/15-likelihood.md."""
    ldl = (v // 8 + 1) * 8 if pitch == "vec" else v + 3
    check_token_nll(dev, rows, v, ldl, dtype, seed=rows * 4099 + v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("v,ldl", [(1024, 1032), (1025, 1032), (2048, 2056), (2049, 2056), (3001, 3008), (1027, 1027)])
def test_token_nll_path_thresholds(dev, v, ldl, dtype):
    """the sizes at which dvq_token_nll changes kernels: 2 / 4 register vectors per lane (V <= 1024 / <= 2048), the one-pass kernel
    beyond 2048 columns, and a row pitch equal to V (no padding column at all)"""
    check_token_nll(dev, 9, v, ldl, dtype, seed=v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("v,ldl", [(65, 72), (1027, 1030)])
def test_token_nll_all_rows_ignored(dev, v, ldl, dtype):
    err, yard = check_token_nll(dev, 7, v, ldl, dtype, seed=5, all_ignored=True)
    assert err == 0.0 and yard == 0.0


def test_token_nll_repeat_is_bit_identical_and_rejects_bad_shapes(dev):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import DvqError
    logits, tg, ign = make_rows(130, 1027, 1032, torch.bfloat16, dev, 11)
    a, b = K.token_nll(logits, 1027, tg, ign), K.token_nll(logits, 1027, tg, ign)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(DvqError):
        K.token_nll(logits, 1033, tg, ign)                   # V > row pitch
    with pytest.raises(DvqError):
        K.nll_segment_sums(a[0], a[1], 13, 10, 11)           # split > Tp
    with pytest.raises(DvqError):
        K.nll_segment_sums(a[0], a[1], 13, 11, 3)            # 143 rows != 130


@pytest.mark.parametrize("tp", [5, 64, 200])
@pytest.mark.parametrize("b", [1, 3])
def test_nll_segment_sums(dev, b, tp):
    """fp64 [B, 2, 4] sums over the kernel's own per-row outputs: 1e-12 relative on the nll sums, counts and hits exact, every split in
    {0, 1, Tp-1, Tp}, two launches bit-identical"""
    from dynamicvectorquantization_amd import kernels as K
    g = torch.Generator().manual_seed(b * 1009 + tp)
    rows, v, ign = b * tp, 65, 21
    x = torch.randn(rows, 72, generator=g)
    tg = torch.randint(0, v, (rows,), generator=g)
    x[torch.arange(rows), tg] += torch.rand(rows, generator=g) * 4.0      # targets ranked 0 .. ~30: every class of hit occurs
    tg[torch.rand(rows, generator=g) < 0.25] = ign
    nll, rank = K.token_nll(x.to(dev), v, tg.to(dev), ign)
    n64, rk = nll.cpu().numpy().astype(np.float64).reshape(b, tp), rank.cpu().numpy().reshape(b, tp)
    if tp >= 64:
        assert (rk < 0).any() and (rk == 0).any() and ((rk > 0) & (rk < 5)).any() and (rk >= 5).any()
    for split in (0, 1, tp - 1, tp):
        out = K.nll_segment_sums(nll, rank, b, tp, split)
        again = K.nll_segment_sums(nll, rank, b, tp, split)
        assert out.dtype == torch.float64 and tuple(out.shape) == (b, 2, 4) and torch.equal(out, again)
        got = out.cpu().numpy()
        for i in range(b):
            for seg, (t0, t1) in enumerate(((0, split), (split, tp))):
                live = rk[i, t0:t1] >= 0
                want = [n64[i, t0:t1][live].sum(), live.sum(), (rk[i, t0:t1] == 0).sum(), (live & (rk[i, t0:t1] < 5)).sum()]
                np.testing.assert_allclose(got[i, seg, 0], want[0], rtol=1e-12, atol=0.0)
                assert got[i, seg, 1:].tolist() == [float(w) for w in want[1:]], (i, seg, split)


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def golden_dualformer(dev, kind):
    """the small Dualformer of tests/test_gpu_stage2.py::test_dualformer_forward_golden (weights, images, labels), in the CURRENT
    compute dtype"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from golden_cfg import dualformer_cfg
    from test_oracle_golden import dqvae_state_dict
    thr_json = os.path.join(REPO, "scripts/tools/thresholds/entropy_thresholds_imagenet_train_patch-16.json")
    target = {"uncond": "models.stage2_dynamic.dqtransformer_uncond_entropy.Dualformer",
              "class": "models.stage2_dynamic.dqtransformer_class2_entropy.Dualformer"}[kind]
    model = instantiate_from_config({"target": target, "params": dualformer_cfg(kind, thr_json)}).to(dev)
    model.first_stage_model.load_state_dict(dqvae_state_dict(load_golden("dqvae_small"), "spread", 512, 64))
    with torch.no_grad():
        for n, p in model.transformer.named_parameters():
            v = synth.det_param(f"dualformer.{kind}." + n, tuple(p.shape))
            p.copy_(torch.from_numpy(v * (0.3 if n == "pos_emb" else 1.0)).to(dev))
    rt.bump_weights_epoch()
    batch = {"image": torch.from_numpy(synth.ragged_grain_images(64, seed=31)).to(dev),
             "class_label": torch.tensor([3, 0, 9], dtype=torch.long, device=dev)}
    return model, batch


def host_token_counts(model, x, c):
    """[B, 4] non-ignored targets per image and stream, counted on the host from teacher_forcing_inputs (activate_pad_ignore models:
    the three pad codes are the ignore indices)"""
    with torch.no_grad():
        _, z = model.encode_to_z(x)
        inp = model.teacher_forcing_inputs(z, model.encode_to_c(c))
    tr = model.transformer
    assert tr.activate_pad_ignore
    cc, fc = inp["coarse_content"].cpu().numpy(), inp["fine_content"].cpu().numpy()
    ct = inp["content_target"].cpu().numpy()
    assert np.array_equal(ct, np.concatenate([cc, fc], 1)[:, 1:])
    cpt, fpt = inp["coarse_position_target"].cpu().numpy(), inp["fine_position_target"].cpu().numpy()
    return np.stack([(cc[:, 1:] != tr.content_pad_code).sum(1), (fc != tr.content_pad_code).sum(1),
                     (cpt != tr.coarse_position_pad_code).sum(1), (fpt != tr.fine_position_pad_code).sum(1)], 1), inp


def recombine(s):
    """[B, 4, 4] sums -> the training step's three batch-mean losses"""
    from dynamicvectorquantization_amd import evaluate as E
    return E.step_losses(np.asarray(s, dtype=np.float64).sum(axis=0))


@pytest.mark.parametrize("kind", ["uncond", "class"])
def test_dualformer_score_fp32(dev, kind):
    """fp32, ragged 3-image golden batch: the per-stream sums recombine to the reference's golden losses (3e-4, the golden test's fp32
    tolerance) and to the model's own with-loss forward in eval mode (1e-5); token counts equal the host count of non-ignored targets;
    training flags are left as found.
    Batch against single images: in a RAGGED batch the shorter coarse streams are padded in the MIDDLE of the sequence (the fine
    stream starts after the longest coarse stream), the pad rows are attended and every later row gets another position embedding -- the
    model itself computes another function of the image there, in the reference as much as here, so no rounding bound applies and only
    the exact token counts are compared.  Scoring equals single-image scoring where the lengths agree: an equal-length batch
    (synth.half_flat_images: every image 8 coarse + 32 fine codes) must match to 1e-5 relative on the nll sums -- the same logits up to
    how the fp32 kernels tile B * Tp rows, the class of difference the with-loss forward is allowed above -- with exact counts and hits."""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import synth
    g = load_golden("dualformer")
    with rt.compute_dtype_ctx(torch.float32):
        model, batch = golden_dualformer(dev, kind)
        model.train()
        x, c = model.get_xc(batch)
        flags = {n: m.training for n, m in model.named_modules()}
        assert model.transformer.training and not model.first_stage_model.training
        s = model.score(x, c)
        assert {n: m.training for n, m in model.named_modules()} == flags
        assert s.dtype == torch.float64 and tuple(s.shape) == (3, 4, 4) and s.is_cuda
        s = s.cpu().numpy()
        got = recombine(s)
        for k in ("content_loss", "coarse_position_loss", "fine_position_loss"):
            print(kind, k, got[k], float(g[f"{kind}.train_{k}"]))
            np.testing.assert_allclose(got[k], float(g[f"{kind}.train_{k}"]), rtol=3e-4)
        model.eval()
        with torch.no_grad():
            own = model(x, c)
        s_eval = model.score(x, c).cpu().numpy()
        assert not model.transformer.training and np.array_equal(s_eval, s)     # train or eval mode outside: the same bits
        for k in ("content_loss", "coarse_position_loss", "fine_position_loss", "position_loss"):
            np.testing.assert_allclose(got[k], float(own[k]), rtol=1e-5)
        counts, _ = host_token_counts(model, x, c)
        assert np.array_equal(s[:, :, 1], counts.astype(np.float64)), (s[:, :, 1], counts)
        assert (s[:, :, 2] <= s[:, :, 3]).all() and (s[:, :, 3] <= s[:, :, 1]).all() and (s[:, :, 0] > 0).all()
        assert len(set(counts[:, 0])) > 1 and len(set(counts[:, 1])) > 1                      # the batch IS ragged
        for i in range(3):
            si = model.score(x[i:i + 1], c[i:i + 1]).cpu().numpy()
            assert np.array_equal(si[0, :, 1], s[i, :, 1])
        # equal lengths: batch == singles
        xe = torch.from_numpy(synth.half_flat_images(3, 64, seed=11)).to(dev)
        ce = xe if kind == "uncond" else c
        ne, _ = host_token_counts(model, xe, ce)
        assert (ne == ne[0]).all(), ne
        se = model.score(xe, ce).cpu().numpy()
        for i in range(3):
            si = model.score(xe[i:i + 1], ce[i:i + 1]).cpu().numpy()[0]
            print(kind, "batch vs single, image", i, float(np.abs(si[:, 0] / se[i, :, 0] - 1).max()))
            np.testing.assert_allclose(si[:, 0], se[i, :, 0], rtol=1e-5)
            assert np.array_equal(si[:, 1:], se[i, :, 1:])


def test_stackgpt_score_split_follows_the_coarse_stream(dev):
    """StackGPT.score on the stackgpt fixture's ragged teacher-forcing batch (coarse streams of 8 + 1 columns, not 256): counts per
    stream equal the host counts, the sums recombine to the with-loss forward"""
    from dynamicvectorquantization_amd import runtime as rt
    from test_gpu_stage2 import build_stackgpt, stackgpt_inputs
    with rt.compute_dtype_ctx(torch.float32):
        model = build_stackgpt(dev).eval()
        raw = stackgpt_inputs()
        inp = {k: torch.from_numpy(v).to(dev) for k, v in raw.items()}
        s = model.score(**inp).cpu().numpy()
        with torch.no_grad():
            own = model(**inp)
    want = np.stack([(raw["coarse_content"][:, 1:] != 1024).sum(1), (raw["fine_content"] != 1024).sum(1),
                     (raw["coarse_position_target"] != 256).sum(1), (raw["fine_position_target"] != 1024).sum(1)], 1)
    assert np.array_equal(s[:, :, 1], want.astype(np.float64))
    got = recombine(s)
    for k in ("content_loss", "coarse_position_loss", "fine_position_loss", "position_loss"):
        np.testing.assert_allclose(got[k], float(own[k]), rtol=1e-5)


def test_dualformer_score_bf16(dev):
    """bf16: finite values, exact token counts, and a repeat that is bit-identical.  The repeat is taken on the same code sequences
    (StackGPT.score twice): the frozen DQ-VAE in front sums its GroupNorm statistics with float atomics, which is outside the scoring
    path"""
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(torch.bfloat16):
        model, batch = golden_dualformer(dev, "uncond")
        model.eval()
        x, c = model.get_xc(batch)
        counts, inp = host_token_counts(model, x, c)
        a, b = model.transformer.score(**inp), model.transformer.score(**inp)
        assert torch.equal(a, b)
        a = a.cpu().numpy()
        assert np.isfinite(a).all() and np.array_equal(a[:, :, 1], counts.astype(np.float64))
        s = model.score(x, c).cpu().numpy()
        assert np.isfinite(s).all() and np.array_equal(s[:, 2:, 1], counts[:, 2:].astype(np.float64))   # positions never flip in bf16
        assert np.array_equal(s[:, :2, 1].sum(1), counts[:, :2].sum(1).astype(np.float64))


def test_evaluate_likelihood_and_meter(dev):
    """evaluate_likelihood over two batches == aggregate_likelihood of the concatenated score blocks; class model through dict batches"""
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(torch.float32):
        model, batch = golden_dualformer(dev, "class")
        model.eval()
        halves = [{k: v[:2] for k, v in batch.items()}, {k: v[2:] for k, v in batch.items()}]
        s = E.evaluate_likelihood(model, halves, per_image=True)
        blocks = [model.score(*model.get_xc(h)).cpu().numpy() for h in halves]
        with pytest.raises(ValueError):
            E.evaluate_likelihood(model, [batch["image"]])
    per = s.pop("per_image")
    assert per.shape == (3, 4, 4) and per.dtype == np.float64 and np.array_equal(per, np.concatenate(blocks, 0))
    want = E.aggregate_likelihood(per, 64 * 64 * 3, model.content_loss_weight, model.position_loss_weight, batch_sizes=[2, 1])
    assert s["dtype"] == "fp32" and {k: v for k, v in s.items() if k != "dtype"} == want
    assert s["position_loss_weight"] == 0.7 and s["pixels_per_image"] == 12288 and s["bits_per_pixel"] > 0
    json.dumps(s)


def test_script_end_to_end(dev, tmp_path):
    """scripts/tools/eval_likelihood.py on synthetic images with the tiny stage-2 config of tests/test_gpu_stage2.py (random weights):
    one JSON line, --json file, --per_image array [N, 4, 4]"""
    import yaml
    from test_gpu_stage2 import dualformer_config
    cfg = tmp_path / "tiny_stage2.yml"
    cfg.write_text(yaml.safe_dump({"model": dualformer_config()}))
    per, js = tmp_path / "per.npy", tmp_path / "out.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts/tools/eval_likelihood.py"), "--yaml_path", str(cfg), "--synthetic", "5",
                        "--batch_size", "2", "--dtype", "fp32", "--per_image", str(per), "--json", str(js)],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    s = json.loads(r.stdout.strip().splitlines()[-1])
    assert s == json.loads(js.read_text())
    a = np.load(per)
    assert a.shape == (5, 4, 4) and a.dtype == np.float64 and np.isfinite(a).all()
    assert s["n_images"] == 5 and s["dtype"] == "fp32" and s["pixels_per_image"] == 64 * 64 * 3
    assert tuple(s["streams"]) == ("content_coarse", "content_fine", "position_coarse", "position_fine")
    assert s["streams"]["content_coarse"]["tokens"] == int(a[:, 0, 1].sum()) == 5 * 9          # 8 coarse codes + <eos> per image
    assert s["streams"]["content_fine"]["tokens"] == 5 * 34                                    # <sos> row's target .. <eos>: 32 codes + 2
    np.testing.assert_allclose(s["nats_per_image"], a[:, :, 0].sum() / 5, rtol=1e-12)
    assert s["loss"]["loss"] is not None and s["loss_batch_mean"]["loss"] is not None
