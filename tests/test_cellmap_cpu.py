"""Host-side tests of the per-cell maps (docs/design/30-cell-maps.md): the numpy restatements of tests/cellmap_math.py against the
per-image restatement of tests/test_eval_cpu.py and the permuter oracle, the Spearman / decile helpers on worked examples with ties,
the host aggregation, and the --maps file."""
import importlib.util
import os

import numpy as np
import pytest

import cellmap_math as CM
from dynamicvectorquantization_amd import evaluate as E
from oracle import permuter as operm
from test_eval_cpu import recon_metrics_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SHAPES = [s for s in CM.RECON_SHAPES if s[0] <= 64]


# ---- reconstruction cells ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("kind", CM.RECON_KINDS)
@pytest.mark.parametrize("h,w,hg,wg", SMALL_SHAPES)
def test_restated_cells_sum_to_the_per_image_restatement(h, w, hg, wg, kind, quantize):
    x, y = CM.image_pair(kind, 2, h, w, seed=h + w + hg)
    cells = CM.recon_cells_ref(x, y, hg, wg, quantize)
    mse, l1, ssim = recon_metrics_ref(x, y, quantize)
    np.testing.assert_allclose(cells[..., 0].sum(axis=(1, 2)) / (3.0 * h * w), mse, rtol=1e-12)
    np.testing.assert_allclose(cells[..., 1].sum(axis=(1, 2)) / (3.0 * h * w), l1, rtol=1e-12)
    np.testing.assert_allclose(cells[..., 2].sum(axis=(1, 2)) / (3.0 * (h - 10) * (w - 10)), ssim, rtol=1e-12)
    assert (cells[..., 2][:, CM.window_counts(h, w, hg, wg) == 0] == 0).all()


@pytest.mark.parametrize("h,w,hg,wg", CM.RECON_SHAPES + [(8, 8, 2, 2), (22, 33, 2, 3)])
def test_window_counts_from_the_geometry(h, w, hg, wg):
    want = CM.window_counts(h, w, hg, wg)
    assert np.array_equal(E.cell_window_counts(h, w, hg, wg), want)
    assert want.sum() == max(h - 10, 0) * max(w - 10, 0)


def test_window_counts_of_the_issue_s_shapes():
    assert E.cell_window_counts(16, 16, 1, 1).tolist() == [[36]]
    assert E.cell_window_counts(32, 32, 2, 2).tolist() == [[256, 96], [96, 36]]
    edge = E.cell_window_counts(32, 32, 4, 4)
    assert (edge[3] == 0).all() and (edge[:, 3] == 0).all() and edge[2, 2] == 36 and edge[0, 0] == 64


def test_float32_restatement_is_close_and_its_yardstick_is_stable():
    """the float32 restatement differs from fp64 by fp32 rounding only; the yardstick over the small shapes is what the design note
    records (the product shape is added on the GPU side's module fixture)"""
    y = CM.ssim_f32_yardstick(SMALL_SHAPES)
    print("fp32 vs fp64 per-cell-mean SSIM deviation, small shapes:", y)
    assert 0.0 < y < 1e-3


# ---- likelihood cells ----------------------------------------------------------------------------------------------------------------
PADS = dict(content_pad=512, content_eos=513, cpos_pad=16, cpos_eos=17, fpos_pad=64, fpos_eos=65)
SOS = dict(coarse=514, coarse_pos=18, fine=514, fine_pos=66)


def teacher_rows(grain, order, seed, tp_extra=3):
    """a ragged batch through the permuter oracle, start tokens in front, and the three target vectors of StackGPT._targets in
    activate_pad_ignore mode with random per-row nll / rank (ignored rows: nll 0, rank -1)"""
    rng = np.random.default_rng(seed)
    b, hw1 = grain.shape[0], grain.shape[1]
    idx = rng.integers(0, 512, (b, hw1 * 2, hw1 * 2))
    z = operm.forward(idx, grain, hw1, 2, order, **PADS)
    col = lambda v: np.full((b, 1), v, dtype=np.int64)
    inputs = {"coarse_content": np.concatenate([col(SOS["coarse"]), z["coarse_content"]], 1),
              "fine_content": np.concatenate([col(SOS["fine"]), z["fine_content"]], 1),
              "coarse_position": np.concatenate([col(SOS["coarse_pos"]), z["coarse_position"]], 1),
              "fine_position": np.concatenate([col(SOS["fine_pos"]), z["fine_position"]], 1)}
    lc, lf = inputs["coarse_content"].shape[1], inputs["fine_content"].shape[1]
    t = lc + lf - 1
    tp = t + tp_extra
    tc = np.full((b, tp), PADS["content_pad"], dtype=np.int64)
    tc[:, :t] = np.concatenate([inputs["coarse_content"], inputs["fine_content"]], 1)[:, 1:]
    tcp = np.full((b, tp), PADS["cpos_pad"], dtype=np.int64)
    tcp[:, :lc - 1] = inputs["coarse_position"][:, 1:]
    tfp = np.full((b, tp), PADS["fpos_pad"], dtype=np.int64)
    tfp[:, lc - 1:t] = inputs["fine_position"]
    rows = {}
    for name, tg, ign in (("content", tc, PADS["content_pad"]), ("coarse_position", tcp, PADS["cpos_pad"]), ("fine_position", tfp, PADS["fpos_pad"])):
        live = tg != ign
        rows[name] = (np.where(live, rng.uniform(0.1, 9.0, tg.shape), 0.0), np.where(live, rng.integers(0, 9, tg.shape), -1), tg)
    return idx, inputs, rows


def mixed_grain(hw1=4, seed=0):
    """all-coarse, all-fine and mixed images in one batch: the row lengths differ and padding rows exist"""
    rng = np.random.default_rng(seed)
    return np.stack([np.zeros((hw1, hw1), dtype=np.int64), np.ones((hw1, hw1), dtype=np.int64), rng.integers(0, 2, (hw1, hw1))])


@pytest.mark.parametrize("order", ["region-first", "row-first"])
def test_restated_forward_back_is_the_oracle_s(order):
    grain = mixed_grain(seed=3)
    idx, inputs, _ = teacher_rows(grain, order, seed=5)
    args = [inputs[k][:, 1:] for k in ("coarse_content", "fine_content", "coarse_position", "fine_position")]
    got, ccell, fcell = CM.forward_back(*args, 4, 2, PADS["cpos_eos"], PADS["fpos_eos"])
    assert np.array_equal(got, operm.forward_back(*args, 4, 2, PADS["cpos_eos"], PADS["fpos_eos"]))
    # with the start tokens in front (what the transformer sees) the map is the same: they are no grid positions
    full = [inputs[k] for k in ("coarse_content", "fine_content", "coarse_position", "fine_position")]
    got2, ccell2, fcell2 = CM.forward_back(*full, 4, 2, PADS["cpos_eos"], PADS["fpos_eos"])
    assert np.array_equal(got2, got) and np.array_equal(ccell2[:, 1:], ccell) and np.array_equal(fcell2[:, 1:], fcell)
    assert (ccell2[:, 0] == -1).all() and (fcell2[:, 0] == -1).all()
    for i in range(3):                                            # every cell is written by the entries its grain says
        g = grain[i].reshape(-1)
        assert sorted(ccell[i][ccell[i] >= 0].tolist()) == np.flatnonzero(g == 0).tolist()
        assert sorted(fcell[i][fcell[i] >= 0].tolist()) == np.repeat(np.flatnonzero(g == 1), 4).tolist()


@pytest.mark.parametrize("order", ["region-first", "row-first"])
def test_token_counts_per_cell_follow_from_the_grain_map(order):
    grain = mixed_grain(seed=7)
    _, inputs, rows = teacher_rows(grain, order, seed=11)
    cells, outside = CM.nll_cells_ref(rows, inputs, 4, 2, PADS["cpos_eos"], PADS["fpos_eos"])
    assert np.array_equal(cells[..., 1], CM.grain_token_counts(grain))
    # outside: the coarse <eos> (content and position), the fine stream's start token and <eos> (content and position)
    assert np.array_equal(outside[:, :, 1], np.tile([1.0, 2.0, 1.0, 2.0], (3, 1)))
    # nothing is lost: cells + outside = the per-stream sums over the live rows
    lc = inputs["coarse_content"].shape[1]
    nll, rank, _ = rows["content"]
    live = rank >= 0
    np.testing.assert_allclose(cells[:, 0, :, 0].sum(1) + outside[:, 0, 0], (nll * live)[:, :lc - 1].sum(1), rtol=1e-13)
    np.testing.assert_allclose(cells[:, 1, :, 0].sum(1) + outside[:, 1, 0], (nll * live)[:, lc - 1:].sum(1), rtol=1e-13)
    for name, s in (("coarse_position", 2), ("fine_position", 3)):
        nll, rank, _ = rows[name]
        np.testing.assert_allclose(cells[:, s, :, 0].sum(1) + outside[:, s, 0], (nll * (rank >= 0)).sum(1), rtol=1e-13)
        assert np.array_equal(cells[:, s, :, 2].sum(1) + outside[:, s, 2], (rank == 0).sum(1).astype(np.float64))


def test_both_fine_orders_give_the_same_cells_for_the_same_tokens():
    """the order changes where a fine token sits in the sequence, not its cell: with nll = the token's own code the maps agree"""
    grain = mixed_grain(seed=9)
    maps = []
    for order in ("region-first", "row-first"):
        _, inputs, rows = teacher_rows(grain, order, seed=13)
        nll, rank, tg = rows["content"]
        rows["content"] = (np.where(rank >= 0, tg.astype(np.float64), 0.0), np.where(rank >= 0, 0, -1), tg)
        maps.append(CM.nll_cells_ref(rows, inputs, 4, 2, PADS["cpos_eos"], PADS["fpos_eos"])[0][:, :2])
    assert np.array_equal(maps[0], maps[1])


# ---- host statistics -----------------------------------------------------------------------------------------------------------------
def test_average_ranks_and_spearman_worked_examples():
    assert E.average_ranks([3, 1, 3, 2]).tolist() == [3.5, 1.0, 3.5, 2.0]
    assert E.average_ranks([5, 5, 5]).tolist() == [2.0, 2.0, 2.0]
    # x ranks (1, 2.5, 2.5, 4), y ranks (1, 3, 2, 4): covariance 4.5, variances 4.5 and 5 -> 4.5 / sqrt(22.5)
    assert E.spearman([1, 2, 2, 3], [1, 3, 2, 4]) == pytest.approx(4.5 / np.sqrt(22.5), abs=1e-15)
    assert E.spearman([1, 2, 2, 3], [10, 20, 20, 30]) == pytest.approx(1.0, abs=1e-15)
    assert E.spearman([1, 2, 3, 4], [9, 7, 5, 0]) == pytest.approx(-1.0, abs=1e-15)
    # no ties: 1 - 6 sum d^2 / (n (n^2 - 1)), d = (0, -1, 1, 0)
    assert E.spearman([1, 2, 3, 4], [1, 3, 2, 4]) == pytest.approx(1.0 - 6.0 * 2.0 / 60.0, abs=1e-15)
    assert E.spearman([1, 1, 1], [1, 2, 3]) is None and E.spearman([1], [2]) is None
    with pytest.raises(ValueError):
        E.spearman([1, 2], [1, 2, 3])


def test_decile_index_worked_examples():
    idx, edges = E.decile_index(np.arange(20))
    assert idx.tolist() == [d for d in range(10) for _ in range(2)]
    # ten zeros then 1 .. 10: the first four inner edges are 0, so every zero lands in decile 4 and deciles 0 .. 3 stay empty
    v = np.array([0] * 10 + list(range(1, 11)), dtype=np.float64)
    idx, edges = E.decile_index(v)
    np.testing.assert_allclose(edges, [0, 0, 0, 0, 0.5, 2.4, 4.3, 6.2, 8.1], atol=1e-12)
    assert idx.tolist() == [4] * 10 + [5, 5, 6, 6, 7, 7, 8, 8, 9, 9]
    perm = np.random.default_rng(0).permutation(20)
    assert E.decile_index(v[perm])[0].tolist() == idx[perm].tolist()


def test_aggregate_cells_hand_built():
    h = w = 32
    grain = np.array([[[0, 1], [1, 0]]])
    recon = np.zeros((1, 2, 2, 3))
    recon[0, :, :, 0] = [[6.0, 1.0], [2.0, 3.0]]
    recon[0, :, :, 2] = 3.0 * E.cell_window_counts(h, w, 2, 2) * np.array([[0.5, 0.9], [0.8, 0.6]])
    ent = np.array([[[0.1, 0.9], [0.8, 0.2]]])
    bits = np.zeros((1, 4, 4, 4))
    ln2 = np.log(2.0)
    bits[0, 0, [0, 3], 0], bits[0, 0, [0, 3], 1] = [2 * ln2, 4 * ln2], 1.0
    bits[0, 1, [1, 2], 0], bits[0, 1, [1, 2], 1] = [8 * ln2, 16 * ln2], 4.0
    outside = np.zeros((1, 4, 4))
    outside[0, 0, :2] = [10 * ln2, 1.0]
    s = E.aggregate_cells(h, w, 2, grain, recon, ent, bits, outside)
    c, f = s["by_grain"]
    assert (c["cells"], f["cells"]) == (2, 2) and c["cell_share"] == 0.5
    assert c["token_share"] == pytest.approx(2 / 10) and f["token_share"] == pytest.approx(8 / 10)
    assert c["sq_err_share"] == pytest.approx(9 / 12) and f["sq_err_share"] == pytest.approx(3 / 12)
    assert c["mse"] == pytest.approx(9.0 / (2 * 16 * 16 * 3)) and c["psnr"] == pytest.approx(10 * np.log10(1 / c["mse"]))
    assert c["ssim"] == pytest.approx((256 * 0.5 + 36 * 0.6) / 292) and f["ssim"] == pytest.approx((0.9 + 0.8) / 2)
    assert c["bits_share"] == pytest.approx(6 / 30) and f["bits_share"] == pytest.approx(24 / 30)
    assert c["bits_per_token"]["content_coarse"] == pytest.approx(3.0) and f["bits_per_token"]["content_fine"] == pytest.approx(3.0)
    assert c["bits_per_token"]["content_fine"] is None and s["outside_bits_share"] == pytest.approx(10 / 40)
    # entropy ranks the cells (0.1, 0.9, 0.8, 0.2); error (6, 1, 2, 3): ranks (1, 4, 3, 2) against (4, 1, 2, 3) -> -1
    assert s["rank_correlation"]["entropy_error"]["pooled"] == pytest.approx(-1.0)
    assert s["rank_correlation"]["entropy_bits"]["pooled"] == pytest.approx(0.8)       # bits (2, 8, 16, 4): ranks (1, 3, 4, 2)
    assert s["rank_correlation"]["bits_error"]["by_grain"] == [pytest.approx(-1.0), pytest.approx(1.0)]
    rows = s["by_entropy_decile"]["rows"]
    assert sum(r["cells"] for r in rows) == 4 and rows[9]["fine_fraction"] == 1.0 and rows[0]["fine_fraction"] == 0.0
    assert rows[9]["bits"] == pytest.approx(8.0) and rows[0]["sq_err"] == pytest.approx(6.0)
    assert s["consistency"]["max"] is None
    # error maps only
    s1 = E.aggregate_cells(h, w, 2, grain, recon, ent)
    assert s1["by_grain"][0]["bits_share"] is None and s1["rank_correlation"]["entropy_bits"] is None
    import json
    json.dumps(s), json.dumps(s1)


def test_consistency_block_against_the_per_image_restatement():
    h, w, hg, wg = 48, 80, 3, 5
    x, y = CM.image_pair("random", 2, h, w, seed=1)
    cells = CM.recon_cells_ref(x, y, hg, wg, True)
    grain = np.zeros((2, hg, wg), dtype=np.int64)
    _, inputs, rows = teacher_rows(mixed_grain(seed=2), "region-first", seed=3)
    bits, outside = CM.nll_cells_ref(rows, inputs, 4, 2, PADS["cpos_eos"], PADS["fpos_eos"])
    score = bits.sum(axis=2) + outside
    s = E.aggregate_cells(h, w, 1, grain, cells, None, ref_recon=recon_metrics_ref(x, y, True))
    assert s["consistency"]["max"] <= 1e-12 and s["consistency"]["ssim"] is not None and s["by_entropy_decile"] is None
    s = E.aggregate_cells(64, 64, 2, mixed_grain(seed=2), bits=bits, outside=outside, ref_score=score)
    assert s["consistency"]["nll"] == 0.0 and s["consistency"]["counts_equal"] is True
    score[1, 2, 0] *= 1.0 + 1e-6
    s = E.aggregate_cells(64, 64, 2, mixed_grain(seed=2), bits=bits, outside=outside, ref_score=score)
    assert s["consistency"]["max"] == pytest.approx(1e-6, rel=1e-3)


def test_maps_file_round_trips(tmp_path):
    h, w, hg, wg = 32, 32, 4, 4
    x, y = CM.image_pair("smooth", 3, h, w, seed=4)
    cells = CM.recon_cells_ref(x, y, hg, wg, True)
    grain = mixed_grain(seed=5)
    _, inputs, rows = teacher_rows(grain, "row-first", seed=6)
    bits, outside = CM.nll_cells_ref(rows, inputs, 4, 2, PADS["cpos_eos"], PADS["fpos_eos"])
    ent = np.random.default_rng(7).uniform(0, 3, (3, hg, wg))
    maps = E.cell_maps(h, w, grain, cells, ent, bits, outside)
    assert set(maps) == {"grain", "image_size", "sq_err", "abs_err", "ssim", "entropy", "bits", "tokens", "outside"}
    assert maps["bits"].shape == (3, 4, 4, 4) and np.isnan(maps["ssim"][:, 3, :]).all() and np.isfinite(maps["ssim"][:, :3, :3]).all()
    np.testing.assert_allclose(maps["bits"].sum(axis=(2, 3)) * np.log(2.0), bits[..., 0].sum(axis=2), rtol=1e-13)
    path = str(tmp_path / "maps.npz")
    E.save_cell_maps(path, maps)
    back = E.load_cell_maps(path)
    assert set(back) == set(maps)
    for k in maps:
        assert back[k].dtype == maps[k].dtype and np.array_equal(back[k], maps[k], equal_nan=True), k
    with pytest.raises(ValueError):
        E.save_cell_maps(str(tmp_path / "maps.npy"), maps)


def test_script_parses_its_flags():
    spec = importlib.util.spec_from_file_location("analyze_allocation", os.path.join(REPO, "scripts/tools/analyze_allocation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opt = mod.get_parser().parse_args(["--yaml_path", "a.yml", "--model_path", "m.ckpt", "--tokens", "dir", "--maps", "f.npz", "--use_ema",
                                       "--device_jpeg", "--device_png", "--batch_size", "4"])
    assert opt.tokens == "dir" and opt.maps == "f.npz" and opt.use_ema and opt.device_jpeg and opt.device_png
    assert mod.is_stage2(os.path.join(REPO, "configs/stage2/uncond_imagenet_p6c18.yml"))
    assert not mod.is_stage2(os.path.join(REPO, "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"))
