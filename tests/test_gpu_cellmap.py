"""GPU tests of the per-cell maps (docs/design/30-cell-maps.md): dvq_recon_cells against the fp64 restatement and against
dvq_recon_metrics, dvq_nll_cell_sums / StackGPT.score_cells / Dualformer.score_cells against score() and the restated attribution, and
scripts/tools/analyze_allocation.py end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cellmap_math as CM
from conftest import REPO

pytestmark = pytest.mark.gpu


# ---- reconstruction cells ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ssim_bound():
    """4 x the largest per-cell-mean deviation of the numpy float32 restatement from the fp64 one over this module's cases (computed on
    the CPU, never from the kernel): the factor covers another summation order inside the window"""
    y = CM.ssim_f32_yardstick()
    print(f"per-cell-mean SSIM: fp32 restatement vs fp64 {y:.3e}, bound {4 * y:.3e}")
    return 4.0 * y


def recon_case(dev, h, w, hg, wg, kind, quantize, b=2):
    from dynamicvectorquantization_amd import kernels as K
    x, y = CM.image_pair(kind, b, h, w, seed=h * 131 + w + hg)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    cells = K.recon_cells(xd, yd, hg, wg, quantize)
    assert cells.dtype == torch.float64 and tuple(cells.shape) == (b, hg, wg, 3)
    return x, y, xd, yd, cells


@pytest.mark.parametrize("quantize", [False, True], ids=["float", "u8"])
@pytest.mark.parametrize("kind", CM.RECON_KINDS)
@pytest.mark.parametrize("h,w,hg,wg", CM.RECON_SHAPES, ids=lambda v: str(v))
def test_recon_cells_vs_restatement_and_per_image_kernel(dev, ssim_bound, h, w, hg, wg, kind, quantize):
    """squared / absolute error: 1e-12 relative per cell against the fp64 restatement and per image against dvq_recon_metrics (fp64 sums
    of identical terms in another order).  SSIM: per-cell mean within `ssim_bound` of fp64; summed over the cells within the same
    bound times the window count of the per-image kernel's value.  Cells without a window report exactly 0."""
    from dynamicvectorquantization_amd import kernels as K
    x, y, xd, yd, cells = recon_case(dev, h, w, hg, wg, kind, quantize)
    got = cells.cpu().numpy()
    ref = CM.recon_cells_ref(x, y, hg, wg, quantize)
    np.testing.assert_allclose(got[..., 0], ref[..., 0], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got[..., 1], ref[..., 1], rtol=1e-12, atol=0.0)
    mse, l1, ssim = [v.cpu().numpy() for v in K.recon_metrics(xd, yd, quantize)]
    np.testing.assert_allclose(got[..., 0].sum(axis=(1, 2)) / (3.0 * h * w), mse, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got[..., 1].sum(axis=(1, 2)) / (3.0 * h * w), l1, rtol=1e-12, atol=0.0)
    win = CM.window_counts(h, w, hg, wg)
    assert (got[..., 2][:, win == 0] == 0.0).all()
    dev_cell = CM.cell_mean_deviation(got[..., 2], ref[..., 2], h, w, hg, wg)
    nwin = 3.0 * win.sum()
    dev_img = float(np.abs(got[..., 2].sum(axis=(1, 2)) - ssim * nwin).max())
    print(f"recon_cells {h}x{w} grid {hg}x{wg} {kind} u8={quantize}: cell-mean SSIM dev {dev_cell:.3e} (bound {ssim_bound:.3e}), "
          f"image sum dev {dev_img:.3e} (bound {ssim_bound * nwin:.3e})")
    assert dev_cell <= ssim_bound
    assert dev_img <= ssim_bound * nwin


@pytest.mark.parametrize("h,w,hg,wg", [(32, 32, 2, 2), (48, 80, 3, 5), (64, 64, 2, 2), (32, 32, 4, 4)], ids=lambda v: str(v))
def test_recon_cells_repeat_and_batch_independence(dev, h, w, hg, wg):
    """two launches give equal bits; an image's map is the same alone and inside a batch of 5"""
    from dynamicvectorquantization_amd import kernels as K
    x, y, xd, yd, cells = recon_case(dev, h, w, hg, wg, "smooth", True, b=5)
    assert torch.equal(cells, K.recon_cells(xd, yd, hg, wg, True))
    for i in (0, 3):
        alone = K.recon_cells(xd[i:i + 1].contiguous(), yd[i:i + 1].contiguous(), hg, wg, True)
        assert torch.equal(alone[0], cells[i])


def test_recon_cells_unaligned_and_odd_geometry(dev, ssim_bound):
    """a cell width that is no multiple of 4 (the scalar staging path), a cell taller than the tile that is no multiple of it (40 rows:
    parts of 16, 16, 8) and wider than it (72 columns: 64 + 8), and an image smaller than the window (no SSIM anywhere)"""
    from dynamicvectorquantization_amd import kernels as K
    for (h, w, hg, wg) in [(30, 33, 5, 11), (80, 144, 2, 2), (8, 12, 2, 3)]:
        x, y, xd, yd, cells = recon_case(dev, h, w, hg, wg, "random", False)
        got, ref = cells.cpu().numpy(), CM.recon_cells_ref(x, y, hg, wg, False)
        np.testing.assert_allclose(got[..., :2], ref[..., :2], rtol=1e-12, atol=0.0)
        assert CM.cell_mean_deviation(got[..., 2], ref[..., 2], h, w, hg, wg) <= ssim_bound
        assert (got[..., 2][:, CM.window_counts(h, w, hg, wg) == 0] == 0.0).all()


def test_recon_cells_rejects_bad_grids(dev):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import DvqError
    x = torch.zeros(1, 3, 32, 32, device=dev)
    for hg, wg in [(3, 2), (2, 5), (0, 2), (2, -1)]:
        with pytest.raises(DvqError):
            K.recon_cells(x, x, hg, wg)
    with pytest.raises(DvqError):
        K.recon_cells(x, x, 2, 2, ws=torch.empty(8, dtype=torch.uint8, device=dev))


# ---- likelihood cells ----------------------------------------------------------------------------------------------------------------
def mixed_images(dev):
    """an all-coarse, an all-fine and a mixed image: three row lengths in one batch, padding rows in both streams"""
    from dynamicvectorquantization_amd import synth
    x = np.concatenate([synth.half_flat_images(1, 64, seed=41, fine_fraction=0.0), synth.half_flat_images(1, 64, seed=42, fine_fraction=1.0),
                        synth.half_flat_images(1, 64, seed=43, fine_fraction=0.5)], 0)
    return torch.from_numpy(x).to(dev)


def teacher_inputs(model, x, c):
    with torch.no_grad():
        _, z = model.encode_to_z(x)
        return z, model.teacher_forcing_inputs(z, model.encode_to_c(c))


def kernel_rows(tr, inp):
    """the per-row nll / rank of the three losses as score() takes them, with their target vectors, on the host"""
    from dynamicvectorquantization_amd import kernels as K
    with torch.no_grad():
        pl, cl, b, t, tp = tr.fwd(inp["coarse_content"], inp["fine_content"], inp["coarse_position"], inp["fine_position"], inp["coarse_seg"],
                                  inp["fine_seg"], None)
        tg = tr._targets(b, t, tp, inp["coarse_position"].shape[1], inp["content_target"], inp["coarse_position_target"],
                         inp["fine_position_target"], pl.device)
        rows = {}
        for name, logits, v, (tgt, ign) in (("content", cl, tr.config.vocab_size, tg[0]), ("coarse_position", pl, tr.config.fine_position_size, tg[1]),
                                            ("fine_position", pl, tr.config.fine_position_size, tg[2])):
            nll, rank = K.token_nll(logits, v, tgt, ign)
            rows[name] = (nll.cpu().numpy().astype(np.float64).reshape(b, tp), rank.cpu().numpy().reshape(b, tp), tgt.cpu().numpy().reshape(b, tp))
    return rows


def check_cells(model, inp, grain=None):
    """score_cells of the teacher-forcing inputs against score() and against the restatement on the kernel's own rows"""
    tr = model.transformer
    hw1, hw2 = model.hw1, model.hw2
    cells, outside = tr.score_cells(**inp, hw1=hw1, hw2=hw2)
    again = tr.score_cells(**inp, hw1=hw1, hw2=hw2)
    assert torch.equal(cells, again[0]) and torch.equal(outside, again[1])                # repeated launches: equal bits
    b = inp["coarse_content"].shape[0]
    assert cells.dtype == torch.float64 and tuple(cells.shape) == (b, 4, hw1 * hw1, 4) and tuple(outside.shape) == (b, 4, 4)
    score = tr.score(**inp).cpu().numpy()
    cells, outside = cells.cpu().numpy(), outside.cpu().numpy()
    tot = cells.sum(axis=2) + outside
    assert np.array_equal(tot[:, :, 1:], score[:, :, 1:])                                 # counts and hits exactly
    np.testing.assert_allclose(tot[:, :, 0], score[:, :, 0], rtol=1e-10, atol=0.0)
    host = {k: v.cpu().numpy() for k, v in inp.items() if k in ("coarse_content", "fine_content", "coarse_position", "fine_position")}
    want_c, want_o = CM.nll_cells_ref(kernel_rows(tr, inp), host, hw1, hw2, model.coarse_position_eos_code, model.fine_position_eos_code)
    assert np.array_equal(cells[..., 1:], want_c[..., 1:]) and np.array_equal(outside[:, :, 1:], want_o[:, :, 1:])
    np.testing.assert_allclose(cells[..., 0], want_c[..., 0], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(outside[..., 0], want_o[..., 0], rtol=1e-12, atol=0.0)
    if grain is not None:
        assert np.array_equal(cells[..., 1], CM.grain_token_counts(grain))
        assert np.array_equal(outside[:, :, 1], np.tile([1.0, 2.0, 1.0, 2.0], (b, 1)))
    return cells, outside


@pytest.fixture(scope="module")
def models(dev):
    """the small Dualformers of tests/test_gpu_likelihood.py (fp32), built once"""
    from dynamicvectorquantization_amd import runtime as rt
    from test_gpu_likelihood import golden_dualformer
    out = {}
    with rt.compute_dtype_ctx(torch.float32):
        for kind in ("uncond", "class"):
            model, batch = golden_dualformer(dev, kind)
            out[kind] = (model.eval(), batch)
    return out


@pytest.mark.parametrize("order", ["region-first", "row-first"])
@pytest.mark.parametrize("kind", ["uncond", "class"])
def test_score_cells_mixed_batch(dev, models, kind, order):
    """all-coarse + all-fine + mixed image in one batch, both fine position orders, unconditional and class-conditional model:
    cells + outside = score(), per-cell token counts = the grain map's, values = the restatement on the kernel's own nll / rank,
    score_cells_tokens = score_cells, Dualformer.score_cells = StackGPT.score_cells"""
    from dynamicvectorquantization_amd import runtime as rt
    model, batch = models[kind]
    x = mixed_images(dev)
    c = x if kind == "uncond" else batch["class_label"]
    saved = (model.permuter.fine_position_order, model.fine_position_order)
    model.permuter.fine_position_order = model.fine_position_order = order
    try:
        with rt.compute_dtype_ctx(torch.float32):
            z, inp = teacher_inputs(model, x, c)
            grain = model.first_stage_model.encode(x)[3].cpu().numpy()
            assert grain[0].sum() == 0 and grain[1].sum() == 16 and 0 < grain[2].sum() < 16
            assert len({int((inp["coarse_content"][i] != model.content_pad_code).sum()) for i in range(3)}) == 3     # ragged
            cells, outside = check_cells(model, inp, grain)
            a = model.score_cells(x, c)
            t = model.score_cells_tokens(z, c)
            assert np.array_equal(a[0].cpu().numpy(), cells) and np.array_equal(a[1].cpu().numpy(), outside)
            assert torch.equal(a[0], t[0]) and torch.equal(a[1], t[1])
    finally:
        model.permuter.fine_position_order, model.fine_position_order = saved


def test_score_cells_order_moves_rows_not_cells(dev, models):
    """the two fine position orders put a fine token on another row; its cell, and therefore every count per cell, stays"""
    from dynamicvectorquantization_amd import runtime as rt
    model, _ = models["uncond"]
    x = mixed_images(dev)
    counts = []
    saved = (model.permuter.fine_position_order, model.fine_position_order)
    try:
        with rt.compute_dtype_ctx(torch.float32):
            for order in ("region-first", "row-first"):
                model.permuter.fine_position_order = model.fine_position_order = order
                counts.append(model.score_cells(x, x)[0][..., 1].cpu().numpy())
    finally:
        model.permuter.fine_position_order, model.fine_position_order = saved
    assert np.array_equal(counts[0], counts[1])


def test_score_cells_without_pad_ignore(dev, models):
    """activate_pad_ignore off: the content loss counts its pad targets (ignore index -100), which have no grid position and land in
    `outside`; the position targets cover rows [0, lc) / [lc, t).  Sums and restatement as before."""
    from dynamicvectorquantization_amd import runtime as rt
    model, _ = models["uncond"]
    tr = model.transformer
    x = mixed_images(dev)
    with rt.compute_dtype_ctx(torch.float32):
        _, inp = teacher_inputs(model, x, x)
        b = x.shape[0]
        pad = torch.full((b, 1), tr.coarse_position_pad_code, dtype=torch.long, device=dev)
        inp = dict(inp, coarse_position_target=torch.cat([inp["coarse_position"][:, 1:], pad], dim=1),
                   fine_position_target=inp["fine_position"][:, 1:].contiguous())
        tr.activate_pad_ignore = False
        try:
            cells, outside = check_cells(model, inp)
        finally:
            tr.activate_pad_ignore = True
    t = inp["coarse_content"].shape[1] + inp["fine_content"].shape[1] - 1
    n_pad = (inp["content_target"] == tr.content_pad_code).sum(1).cpu().numpy()
    assert n_pad.max() > 0
    assert np.array_equal(cells[:, :2, :, 1].sum(axis=(1, 2)) + outside[:, :2, 1].sum(axis=1), np.full(b, float(t)))     # every row counts
    assert np.array_equal(outside[:, :2, 1].sum(axis=1), n_pad + 3.0)                      # pads + coarse <eos> + fine <sos>, <eos>


def test_nll_cell_sums_arguments(dev):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import DvqError
    b, tp, hw1 = 2, 300, 4
    g = torch.Generator().manual_seed(3)
    nll = torch.rand(b * tp, generator=g).to(dev)
    rank = torch.randint(-1, 9, (b * tp,), generator=g, dtype=torch.int32).to(dev)
    pos = torch.randint(-2, 70, (b * tp,), generator=g).to(dev)
    cells = torch.full((b, 4, hw1 * hw1, 4), -7.0, dtype=torch.float64, device=dev)
    outside = torch.full((b, 4, 4), -7.0, dtype=torch.float64, device=dev)
    K.nll_cell_sums(nll, rank, pos, b, tp, 257, hw1, 2, (-1, 3), cells, outside)          # a segment longer than one 256-row chunk
    assert bool((cells[:, :3] == -7.0).all()) and bool((outside[:, :3] == -7.0).all())    # skipped streams are left alone
    n, r, p = nll.cpu().numpy().astype(np.float64).reshape(b, tp), rank.cpu().numpy().reshape(b, tp), pos.cpu().numpy().reshape(b, tp)
    _, fine_of = CM.code_cells(hw1, 2, 1000, 1001)
    want_c, want_o = np.zeros((b, 16, 4)), np.zeros((b, 4))
    for i in range(b):
        for t in range(257, tp):
            if r[i, t] >= 0:
                tgt = want_c[i, fine_of[p[i, t]]] if 0 <= p[i, t] < 64 else want_o[i]
                tgt += [n[i, t], 1.0, float(r[i, t] == 0), float(r[i, t] < 5)]
    np.testing.assert_allclose(cells[:, 3].cpu().numpy(), want_c, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(outside[:, 3].cpu().numpy(), want_o, rtol=1e-12, atol=0.0)
    with pytest.raises(DvqError):
        K.nll_cell_sums(nll, rank, pos, b, tp, tp + 1, hw1, 2, (0, 1), cells, outside)
    with pytest.raises(DvqError):
        K.nll_cell_sums(nll, rank, pos, b, tp, 5, hw1, 2, (1, 1), cells, outside)
    with pytest.raises(DvqError):
        K.nll_cell_sums(nll, rank, pos.int(), b, tp, 5, hw1, 2, (0, 1), cells, outside)


# ---- host layer and script -----------------------------------------------------------------------------------------------------------
def test_evaluate_cells_stage1_and_stage2(dev, models):
    """evaluate_cells over two batches: error maps alone from the first stage, error + bit maps with the Dualformer; the cells add up to
    evaluate_reconstruction's / score()'s per-image figures"""
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    model, _ = models["uncond"]
    x = mixed_images(dev)
    with rt.compute_dtype_ctx(torch.float32):
        s1 = E.evaluate_cells(model.first_stage_model, [x[:2], x[2:]])
        s2 = E.evaluate_cells(None, [x[:2], x[2:]], stage2=model, maps=True)
    maps = s2.pop("maps")
    json.dumps(s1), json.dumps(s2)
    assert s1["by_grain"][0]["bits_share"] is None and s1["rank_correlation"]["entropy_bits"] is None
    assert s1["consistency"]["max"] <= 1e-9 and s2["consistency"]["max"] <= 1e-9 and s2["consistency"]["counts_equal"] is True
    assert [g["cells"] for g in s2["by_grain"]] == [int((maps["grain"] == 0).sum()), int((maps["grain"] == 1).sum())]
    np.testing.assert_allclose(s1["by_grain"][0]["mse"], s2["by_grain"][0]["mse"], rtol=1e-3)     # two forwards of the first stage
    assert maps["bits"].shape == (3, 4, 4, 4) and maps["entropy"].shape == (3, 4, 4) and maps["outside"].shape == (3, 4, 4)
    assert np.array_equal(maps["tokens"].reshape(3, 4, 16), CM.grain_token_counts(maps["grain"]))
    for k in ("entropy_error", "entropy_bits", "bits_error"):
        assert s2["rank_correlation"][k]["pooled"] is not None
    assert sum(r["cells"] for r in s2["by_entropy_decile"]["rows"]) == 48


def test_evaluate_cells_from_token_batches(dev, models):
    """token batches (what --tokens DIR feeds): bit maps only, no first stage; the grain map read off the fine stream's token counts is
    the encoder's, the maps are score_cells', and the blocks that need error maps or entropies are absent"""
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    model, _ = models["uncond"]
    x = mixed_images(dev)
    with rt.compute_dtype_ctx(torch.float32):
        z, _ = teacher_inputs(model, x, x)
        grain = model.first_stage_model.encode(x)[3].cpu().numpy()
        s = E.evaluate_cells(None, [{"tokens": z}], stage2=model, maps=True)
        cells, outside = model.score_cells_tokens(z, z["coarse_content"])
    maps = s.pop("maps")
    json.dumps(s)
    assert np.array_equal(maps["grain"], grain) and set(maps) == {"grain", "image_size", "bits", "tokens", "outside"}
    assert maps["image_size"].tolist() == [64, 64]
    np.testing.assert_allclose(maps["bits"].reshape(3, 4, 16) * np.log(2.0), cells[..., 0].cpu().numpy(), rtol=1e-13, atol=0.0)
    assert np.array_equal(maps["outside"], outside.cpu().numpy())
    assert s["by_entropy_decile"] is None and s["rank_correlation"]["entropy_bits"] is None and s["by_grain"][0]["mse"] is None
    assert s["by_grain"][1]["bits_share"] > 0 and s["consistency"]["nll"] <= 1e-9 and s["consistency"]["counts_equal"] is True


def test_script_end_to_end(dev, tmp_path):
    """scripts/tools/analyze_allocation.py on 8 synthetic images with the tiny stage-2 config of tests/test_gpu_stage2.py (random
    weights): one JSON line with the four blocks, consistency <= 1e-9, and the --maps file"""
    import yaml
    from test_gpu_stage2 import dualformer_config
    cfg = tmp_path / "tiny_stage2.yml"
    cfg.write_text(yaml.safe_dump({"model": dualformer_config()}))
    maps, js = tmp_path / "maps.npz", tmp_path / "out.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts/tools/analyze_allocation.py"), "--yaml_path", str(cfg), "--synthetic", "8",
                        "--batch_size", "3", "--dtype", "fp32", "--maps", str(maps), "--json", str(js)],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    s = json.loads(lines[-1])
    assert s == json.loads(js.read_text()) and sum(1 for ln in lines if ln.startswith("{")) == 1
    for block in ("by_grain", "by_entropy_decile", "rank_correlation", "consistency"):
        assert s[block] is not None, block
    print("consistency", s["consistency"])
    assert s["consistency"]["max"] <= 1e-9 and s["consistency"]["counts_equal"] is True
    assert s["n_images"] == 8 and s["grid"] == [4, 4] and len(s["by_grain"]) == 2
    assert s["by_grain"][0]["cells"] + s["by_grain"][1]["cells"] == 8 * 16
    from dynamicvectorquantization_amd import evaluate as E
    m = E.load_cell_maps(str(maps))
    assert m["sq_err"].shape == (8, 4, 4) and m["bits"].shape == (8, 4, 4, 4) and m["outside"].shape == (8, 4, 4)
    assert np.array_equal(m["tokens"].reshape(8, 4, 16), CM.grain_token_counts(m["grain"]))
