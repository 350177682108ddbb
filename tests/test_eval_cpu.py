"""Host-side tests of the reconstruction evaluation (docs/design/13-evaluation.md): an fp64 numpy restatement of the metric
definitions (also the reference of tests/test_gpu_eval.py), the token-alignment rule of the code histogram, the host aggregation of
dynamicvectorquantization_amd.evaluate, and the scripts' command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dynamicvectorquantization_amd import calibrate
from dynamicvectorquantization_amd import evaluate as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- fp64 restatement of include/dvq_hip.h, dvq_recon_metrics ------------------------------------------------------------------------
def to01(v, quantize_u8=False):
    d = np.clip(np.asarray(v, dtype=np.float64) * 0.5 + 0.5, 0.0, 1.0)
    return np.floor(d * 255.0 + 0.5) / 255.0 if quantize_u8 else d


def gaussian11():
    k = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def _filt(a):
    """valid separable 11 x 11 Gaussian filter over the last two axes (fp64)"""
    g = gaussian11()
    h, w = a.shape[-2:]
    r = sum(g[k] * a[..., :, k:w - 10 + k] for k in range(11))
    return sum(g[k] * r[..., k:h - 10 + k, :] for k in range(11))


def ssim_terms(x01, y01):
    """luminance and contrast-structure maps of every channel, valid positions only"""
    mx, my = _filt(x01), _filt(y01)
    vx, vy, cxy = _filt(x01 * x01) - mx * mx, _filt(y01 * y01) - my * my, _filt(x01 * y01) - mx * my
    lum = (2 * mx * my + C1) / (mx * mx + my * my + C1)
    cs = (2 * cxy + C2) / (vx + vy + C2)
    return lum, cs


def recon_metrics_ref(x, y, quantize_u8=False):
    """x, y [B,3,H,W] in [-1, 1] -> (mse, l1, ssim) fp64 [B]"""
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    x01, y01 = to01(x64, quantize_u8), to01(y64, quantize_u8)
    mse = ((x01 - y01) ** 2).mean(axis=(1, 2, 3))
    l1 = np.abs(x64 - y64).mean(axis=(1, 2, 3))
    lum, cs = ssim_terms(x01, y01)
    return mse, l1, (lum * cs).mean(axis=(1, 2, 3))


def psnr_ref(mse):
    mse = np.asarray(mse, dtype=np.float64)
    return float(np.mean(10.0 * np.log10(1.0 / mse[mse > 0])))


# ---- token-alignment rule, a plain loop -------------------------------------------------------------------------------------------------
def tokens_loop(codes, grain, n_grains):
    """-> (tokens per image, counts [G, K] as a dict {(g, code): n}) by include/dvq_hip.h's rule"""
    b, hf, wf = codes.shape
    r = hf // grain.shape[1]
    tokens, counts = [], {}
    for n in range(b):
        t = 0
        for i in range(hf):
            for j in range(wf):
                g = int(grain[n, i // r, j // r])
                s = r >> g
                if i % s == 0 and j % s == 0:
                    t += 1
                    key = (g, int(codes[n, i, j]))
                    counts[key] = counts.get(key, 0) + 1
        tokens.append(t)
    return np.array(tokens), counts


def test_ssim_of_identical_images_is_one():
    x = np.random.RandomState(0).uniform(-1, 1, size=(2, 3, 23, 31))
    mse, l1, ssim = recon_metrics_ref(x, x)
    assert np.all(mse == 0) and np.all(l1 == 0)
    np.testing.assert_allclose(ssim, 1.0, rtol=0, atol=1e-12)


def test_ssim_of_constant_images_is_the_luminance_term():
    a, b = 0.3, -0.5
    x, y = np.full((1, 3, 16, 16), a), np.full((1, 3, 16, 16), b)
    _, _, ssim = recon_metrics_ref(x, y)
    ua, ub = a * 0.5 + 0.5, b * 0.5 + 0.5
    np.testing.assert_allclose(ssim, (2 * ua * ub + C1) / (ua * ua + ub * ub + C1), rtol=1e-12)
    mse, _, _ = recon_metrics_ref(x, y)
    np.testing.assert_allclose(mse, (ua - ub) ** 2, rtol=1e-12)


def test_sigma_terms_are_invariant_to_a_common_shift():
    rs = np.random.RandomState(1)
    x01 = rs.uniform(0.2, 0.6, size=(2, 3, 20, 20))
    y01 = np.clip(x01 + 0.05 * rs.standard_normal(x01.shape), 0.0, 0.7)
    lum, cs = ssim_terms(x01, y01)
    lum2, cs2 = ssim_terms(x01 + 0.25, y01 + 0.25)
    np.testing.assert_allclose(cs2, cs, rtol=1e-9, atol=1e-12)
    assert not np.allclose(lum2, lum, rtol=1e-6)            # the luminance term does move


def test_quantization_matches_png_rounding():
    v = np.array([-1.0, 1.0, 0.0, 2.0, -3.0, 2.0 / 255.0 - 1.0], dtype=np.float32)
    q = to01(v, True) * 255.0
    assert np.array_equal(q, [0, 255, 128, 255, 0, 1])


def test_token_rule_dual_matches_sequence_length_stats():
    rs = np.random.RandomState(2)
    grain = rs.randint(0, 2, size=(5, 16, 16))
    grain[0] = 0
    grain[1] = 1
    codes = rs.randint(0, 1024, size=(5, 32, 32))
    tokens, counts = tokens_loop(codes, grain, 2)
    seq = (1 * (grain == 0) + 4 * (grain == 1)).reshape(5, -1).sum(axis=1)
    assert np.array_equal(tokens, seq)
    st = calibrate.sequence_length_stats(grain)
    assert E.tokens_stats(tokens) == {"mean": st["mean"], "variance": st["variance"], "min": st["min"], "max": st["max"]}
    assert tokens[0] == 256 and tokens[1] == 1024
    assert sum(n for (g, _), n in counts.items() if g == 1) == 4 * int((grain == 1).sum())


def test_token_rule_triple_hand_built():
    grain = np.array([[[0, 1], [2, 0]]])                    # 2 x 2 cells of 4 x 4 codes: 1 + 4 + 16 + 1 tokens
    codes = np.arange(64).reshape(1, 8, 8)
    tokens, counts = tokens_loop(codes, grain, 3)
    assert tokens.tolist() == [22]
    by_grain = {g: sorted(c for (gg, c) in counts if gg == g) for g in range(3)}
    assert by_grain[0] == [0, 36]                           # top-left code of each coarse cell
    assert by_grain[1] == [4, 6, 20, 22]                    # every second row / column of the median cell
    assert by_grain[2] == [r * 8 + c for r in range(4, 8) for c in range(4)]


def test_aggregate_perplexity_usage_and_exact_images():
    counts = np.zeros((2, 8), dtype=np.int64)
    counts[0, :4] = 5                                       # grain 0: four codes, uniform
    counts[1, 2] = 8                                        # grain 1: code 2 only, 8 tokens = 2 cells
    mse = np.array([0.0, 1e-2, 1e-4])
    s = E.aggregate(mse, [0.0, 0.1, 0.2], [1.0, 0.5, 0.9], counts, [9, 12, 7], invalid=3)
    assert s["n_images"] == 3 and s["n_exact"] == 1
    assert s["psnr"] == pytest.approx((20.0 + 40.0) / 2, abs=1e-12)
    assert s["mse"] == pytest.approx(np.mean(mse)) and s["l1"] == pytest.approx(0.1) and s["ssim"] == pytest.approx(0.8)
    assert s["codes_used"] == 4
    assert s["used_fraction"] == 0.5 and s["unused_fraction"] == 0.5 and s["reference_usage"] == 0.5
    p = np.array([5, 5, 13, 5]) / 28.0
    assert s["perplexity"] == pytest.approx(float(np.exp(-(p * np.log(p)).sum())), rel=1e-12)
    assert s["per_grain"][0] == {"tokens": 20, "codes_used": 4, "perplexity": pytest.approx(4.0, rel=1e-12)}
    assert s["per_grain"][1] == {"tokens": 8, "codes_used": 1, "perplexity": pytest.approx(1.0)}
    assert s["grain_fraction"] == pytest.approx([20 / 22, 2 / 22])
    assert s["tokens_per_image"] == {"mean": pytest.approx(28 / 3), "variance": pytest.approx(np.var([9, 12, 7])), "min": 7, "max": 12}
    assert s["invalid"] == 3
    assert s["lpips"] is None and "lpips_note" in s
    assert E.aggregate([0.0], [0.0], [1.0], counts, [1])["psnr"] is None
    assert E.aggregate([1e-2], [0.0], [1.0], counts, [1], lpips=[0.25])["lpips"] == 0.25


def test_reference_usage_is_the_unused_fraction():
    counts = np.zeros((1, 1024), dtype=np.int64)
    counts[0, :256] = 1
    s = E.aggregate([1e-3], [0.0], [1.0], counts, [256])
    assert s["reference_usage"] == 1 - 256 / 1024 == s["unused_fraction"]
    assert s["perplexity"] == pytest.approx(256.0)


@pytest.mark.parametrize("script", ["codebook_usage_dqvae.py", "eval_reconstruction.py"])
def test_scripts_parse_the_reference_flags(script):
    path = os.path.join(REPO, "scripts", "tools", script)
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--yaml_path", "--model_path", "--batch_size", "--dataset_type", "--codebook_size", "--images", "--synthetic",
                 "--limit", "--dtype"):
        assert flag in r.stdout, flag
    if script == "eval_reconstruction.py":
        assert "--no_quantize_u8" in r.stdout and "--json" in r.stdout and "--dump_dir" in r.stdout
    r = subprocess.run([sys.executable, path, "--yaml_path", "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml", "--dataset_type", "ffhq",
                        "--batch_size", "4", "--codebook_size", "1024"], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 2 and "FFHQ" in r.stderr and "--images" in r.stderr, r.stderr[-2000:]
