"""GPU tests of the reconstruction evaluation (csrc/metrics.hip, dynamicvectorquantization_amd/evaluate.py, the two scripts):
dvq_recon_metrics against the fp64 restatement of tests/test_eval_cpu.py, its determinism, dvq_code_histogram against np.bincount
and the token rule, evaluate_reconstruction end to end on the shrunken dual / triple models.  `pytest -m gpu`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from dynamicvectorquantization_amd import _lib, calibrate, synth
from dynamicvectorquantization_amd import evaluate as E
from dynamicvectorquantization_amd import kernels as K
from test_eval_cpu import psnr_ref, recon_metrics_ref, tokens_loop

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(kind, b, h, w, seed):
    rs = np.random.RandomState(seed)
    if kind == "random":
        x = rs.uniform(-1, 1, size=(b, 3, h, w))
        y = rs.uniform(-1, 1, size=(b, 3, h, w))
    elif kind == "smooth":
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        ph = rs.uniform(0, 6, size=(b, 3, 1, 1))
        x = 0.8 * np.sin(3 * xx + 2 * yy + ph) * np.cos(2 * yy - ph)
        y = x + 0.01 * rs.standard_normal(x.shape)
    else:        # saturated: patches far outside [-1, 1] in both images (clamped to 0 and 1) beside random texture
        x = rs.uniform(-1, 1, size=(b, 3, h, w))
        y = np.clip(x + 0.1 * rs.standard_normal(x.shape), -1.2, 1.2)
        hh, ww = h // 2, w // 2
        x[:, :, :hh, :ww], y[:, :, :hh, :ww] = 1.5, 1.7
        x[:, :, hh:, ww:], y[:, :, hh:, ww:] = -1.3, -2.0
        x[:, 1, hh:, :ww] = -1.5                              # one image saturated, the other not
    return x.astype(np.float32), y.astype(np.float32)


def _gpu(x, y, dev, q):
    mse, l1, ssim = K.recon_metrics(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), q)
    return mse.cpu().numpy(), l1.cpu().numpy(), ssim.cpu().numpy()


@pytest.mark.parametrize("shape", [(4, 256, 256), (3, 64, 64), (3, 37, 53)])
@pytest.mark.parametrize("kind", ["random", "smooth", "saturated"])
@pytest.mark.parametrize("q", [False, True])
def test_recon_metrics_vs_fp64(dev, shape, kind, q):
    x, y = _pair(kind, *shape, seed=sum(shape) + len(kind))
    mse, l1, ssim = _gpu(x, y, dev, q)
    rmse, rl1, rssim = recon_metrics_ref(x, y, q)
    assert mse.dtype == np.float64 and mse.shape == (shape[0],)
    np.testing.assert_allclose(mse, rmse, rtol=1e-6, atol=0)
    np.testing.assert_allclose(l1, rl1, rtol=1e-6, atol=0)
    np.testing.assert_allclose(ssim, rssim, rtol=0, atol=1e-5)


def test_recon_metrics_identical_inputs_and_small_images(dev):
    x, _ = _pair("random", 2, 40, 44, 3)
    for q in (False, True):
        mse, l1, ssim = _gpu(x, x, dev, q)
        assert np.all(mse == 0.0) and np.all(l1 == 0.0)
        np.testing.assert_allclose(ssim, 1.0, rtol=0, atol=1e-6)
    t = torch.zeros(1, 3, 10, 32, device=dev)
    with pytest.raises(_lib.DvqError):
        K.recon_metrics(t, t)
    t = torch.zeros(1, 3, 32, 10, device=dev)
    with pytest.raises(_lib.DvqError):
        K.recon_metrics(t, t)


def test_recon_metrics_deterministic_and_batch_independent(dev):
    x, y = _pair("smooth", 6, 96, 80, 5)
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    a = [t.cpu().numpy() for t in K.recon_metrics(xt, yt, True)]
    b = [t.cpu().numpy() for t in K.recon_metrics(xt, yt, True)]
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    for split in (2, 3):
        parts = [[t.cpu().numpy() for t in K.recon_metrics(xt[i:j].contiguous(), yt[i:j].contiguous(), True)]
                 for i, j in ((0, split), (split, 6))]
        for m in range(3):
            assert np.array_equal(np.concatenate([parts[0][m], parts[1][m]]), a[m]), (split, m)


@pytest.mark.parametrize("layout", [("dual", 32, 16, 2), ("triple", 32, 8, 3), ("single", 32, 32, 1)])
@pytest.mark.parametrize("k", [1024, 8192])
def test_code_histogram_vs_bincount(dev, layout, k):
    _, hf, hg, g = layout
    rs = np.random.RandomState(k + g)
    b = 5
    calls = []
    for _ in range(2):
        codes = rs.randint(0, k, size=(b, hf, hf)).astype(np.int64)
        grain = rs.randint(0, g, size=(b, hg, hg)).astype(np.int64)
        calls.append((codes, grain))
    counts = torch.zeros(g, k, dtype=torch.int64, device=dev)
    invalid = torch.zeros(1, dtype=torch.int64, device=dev)
    want = np.zeros((g, k), dtype=np.int64)
    for codes, grain in calls:
        gt = torch.from_numpy(grain).to(dev) if g > 1 else None
        tokens = K.code_histogram(torch.from_numpy(codes).to(dev), gt, k, g, counts, invalid).cpu().numpy()
        ref_tokens, ref_counts = tokens_loop(codes, grain if g > 1 else np.zeros((b, hf, hf), np.int64), g)
        assert np.array_equal(tokens, ref_tokens)
        for gg in range(g):       # bincount of the codes at the token positions of grain gg
            s = (hf // hg) >> gg
            sel = []
            for n in range(b):
                gm = np.kron(grain[n], np.ones((hf // hg, hf // hg), np.int64)) if g > 1 else np.zeros((hf, hf), np.int64)
                ii, jj = np.meshgrid(np.arange(hf), np.arange(hf), indexing="ij")
                sel.append(codes[n][(gm == gg) & (ii % s == 0) & (jj % s == 0)])
            want[gg] += np.bincount(np.concatenate(sel), minlength=k)
        assert sum(ref_counts.values()) == int(ref_tokens.sum())
    assert np.array_equal(counts.cpu().numpy(), want)           # accumulated over both calls
    assert int(invalid.cpu()[0]) == 0


def test_code_histogram_out_of_range_codes(dev):
    k = 64
    codes = np.zeros((2, 32, 32), dtype=np.int64)
    grain = np.zeros((2, 16, 16), dtype=np.int64)                # all coarse: token positions are the even (i, j)
    codes[0, 0, 0], codes[0, 2, 4], codes[1, 30, 30] = -1, k, k + 100
    codes[1, 1, 1] = k + 5                                       # not a token position: ignored
    counts = torch.zeros(2, k, dtype=torch.int64, device=dev)
    invalid = torch.zeros(1, dtype=torch.int64, device=dev)
    tokens = K.code_histogram(torch.from_numpy(codes).to(dev), torch.from_numpy(grain).to(dev), k, 2, counts, invalid)
    assert tokens.cpu().tolist() == [256, 256]
    assert int(invalid.cpu()[0]) == 3
    c = counts.cpu().numpy()
    assert c[0, 0] == 2 * 256 - 3 and c.sum() == 2 * 256 - 3
    with pytest.raises(_lib.DvqError):                           # a cell of 4 x 4 codes is not 2^(G-1) = 2 codes per side
        K.code_histogram(torch.from_numpy(codes).to(dev), torch.from_numpy(grain[:, :8, :8].copy()).to(dev), k, 2, counts, invalid)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _check_model(dev, model, n_grains, batches):
    before = _state(model)
    s = E.evaluate_reconstruction(model, batches, quantize_u8=True, lpips=False)
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "evaluation changed the model's state"
    recs, codes, grains = [], [], []
    with torch.no_grad():
        for x in batches:
            out = model.ae_fwd(x, None)
            recs.append(out["rec"].cpu().numpy())
            grains.append(out["grain"].cpu().numpy())
            enc = model.encode(x)
            codes.append(enc[2][-1].cpu().numpy())
    xs = np.concatenate([x.cpu().numpy() for x in batches])
    rmse, rl1, rssim = recon_metrics_ref(xs, np.concatenate(recs), True)
    assert s["n_images"] == xs.shape[0] and s["dtype"] == "fp32"
    assert s["psnr"] == pytest.approx(psnr_ref(rmse), abs=1e-5)
    assert s["ssim"] == pytest.approx(float(rssim.mean()), abs=1e-5)
    assert s["mse"] == pytest.approx(float(rmse.mean()), rel=1e-6) and s["l1"] == pytest.approx(float(rl1.mean()), rel=1e-6)
    used = np.unique(np.concatenate([c.reshape(-1) for c in codes]))
    assert s["codes_used"] == used.size
    meter = E.ReconstructionMeter(model.quantize.codebook.n_embed, n_grains)
    with torch.no_grad():
        for x in batches:
            out = model.ae_fwd(x, None)
            meter.update(x, out["rec"], out["codes"], out["grain"])
    assert np.array_equal(np.nonzero(meter.counts.cpu().numpy().sum(axis=0))[0], used)
    g = np.concatenate(grains)
    cells = np.array([(g == v).sum() for v in range(n_grains)], dtype=np.float64)
    assert s["grain_fraction"] == pytest.approx((cells / cells.sum()).tolist(), abs=1e-12)
    assert [p["tokens"] for p in s["per_grain"]] == [int(cells[v]) * 4 ** v for v in range(n_grains)]
    assert s["tokens_per_image"]["mean"] * s["n_images"] == pytest.approx(sum(int(cells[v]) * 4 ** v for v in range(n_grains)))
    assert s["invalid"] == 0 and s["lpips"] is None
    return s, g


def test_evaluate_small_entropy_dual(dev):
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from golden_cfg import dualformer_cfg
    with rt.compute_dtype_ctx("fp32"):
        torch.manual_seed(0)
        model = instantiate_from_config(dualformer_cfg("uncond")["first_stage_config"]).to(dev)
        with torch.no_grad():
            for n, p in model.named_parameters():
                p.copy_(torch.from_numpy(synth.det_param(n, tuple(p.shape))).to(dev))
            cbw = synth.det_param("quantize.codebook.weight.spread", (513, 64)) * np.sqrt(64) * 1.2
            model.quantize.codebook.weight.copy_(torch.from_numpy(cbw).to(dev))
        rt.bump_weights_epoch()
        batches = [torch.from_numpy(synth.half_flat_images(4, 64, seed=s)).to(dev) for s in (7, 8)]
        s, g = _check_model(dev, model, 2, batches)
        assert s["grain_fraction"][1] == pytest.approx(float(g.mean()))        # = the model's train_fine_ratio
        assert s["tokens_per_image"] == calibrate.sequence_length_stats(g)
        assert s["ema_dead_codes"] == model.quantize.codebook.n_embed           # fresh EMA statistics: all zero


def test_evaluate_small_triple(dev):
    from dynamicvectorquantization_amd import runtime as rt
    from test_gpu_featrouted import build_feat
    with rt.compute_dtype_ctx("fp32"):
        model = build_feat("triple", dev, load_golden("featrouted_triple"))
        batches = [torch.from_numpy(synth.half_flat_images(3, 64, seed=s)).to(dev) for s in (21, 22)]
        s, g = _check_model(dev, model, 3, batches)
        n = g.size
        assert s["grain_fraction"][2] == pytest.approx((g == 2).sum() / n)     # fine_radio
        assert s["grain_fraction"][1] == pytest.approx((g == 1).sum() / n)     # median_radio


def _run(script, *args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts/tools", script), "--yaml_path",
                        "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml", *args], capture_output=True, text=True, timeout=timeout,
                       cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_scripts_on_the_shipped_yaml(dev, tmp_path):
    out = _run("codebook_usage_dqvae.py", "--synthetic", "8", "--batch_size", "4", "--codebook_size", "1024")
    lines = out.strip().splitlines()
    assert lines[-1].startswith("usage:  ")
    used = int(lines[-2])
    js = str(tmp_path / "eval.json")
    dump = tmp_path / "dump"
    out = _run("eval_reconstruction.py", "--synthetic", "8", "--batch_size", "4", "--json", js, "--dump_dir", str(dump))
    s = json.loads(out.strip().splitlines()[-1])
    with open(js) as f:
        assert json.load(f) == s
    assert s["codes_used"] == used
    assert float(lines[-1].split()[-1]) == pytest.approx(1 - used / 1024)
    assert s["tokens_per_image"]["mean"] == 640.0 and s["tokens_per_image"]["variance"] == 0.0
    assert s["n_images"] == 8 and s["dtype"] == "bf16"
    assert sorted(os.listdir(dump)) == [f"{i:06d}.png" for i in range(8)]


def test_folder_and_npy_give_identical_metrics(dev, tmp_path):
    from PIL import Image
    folder = tmp_path / "imgs"
    folder.mkdir()
    rs = np.random.RandomState(9)
    for i in range(5):
        Image.fromarray(rs.randint(0, 256, size=(256, 256, 3), dtype=np.uint8), "RGB").save(str(folder / f"im{i}.png"))
    npy = str(tmp_path / "imgs.npy")
    np.save(npy, calibrate.load_images(str(folder), 256))
    a = [t.cpu().numpy() for t in E.image_batches(2, 256, dev, str(folder))]
    b = [t.cpu().numpy() for t in E.image_batches(2, 256, dev, npy)]
    assert [t.shape[0] for t in a] == [2, 2, 1] and all(np.array_equal(u, v) for u, v in zip(a, b))
    res = []
    for src in (str(folder), npy):
        out = _run("eval_reconstruction.py", "--images", src, "--batch_size", "2", "--dtype", "fp32")
        res.append(json.loads(out.strip().splitlines()[-1]))
    # the inputs are bit-identical (above); the forward's GroupNorm statistics are summed with fp64 atomics, so two processes may
    # differ in the last bits of a reconstruction: values to 1e-6, counts exactly
    assert res[0].keys() == res[1].keys()
    for key in ("n_images", "n_exact", "codes_used", "per_grain", "grain_fraction", "tokens_per_image", "invalid", "dtype"):
        assert res[0][key] == res[1][key], key
    for key in ("l1", "mse", "psnr", "ssim", "perplexity"):
        assert res[0][key] == pytest.approx(res[1][key], rel=1e-6), key
