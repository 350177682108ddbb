"""GPU tests of the token shards (docs/design/16-token-shards.md): dvq_tokens_pack / dvq_tokens_unpack against oracle/permuter.py and the
device permuter (exact), their bounds and error paths, Dualformer.score_tokens / forward_tokens and the training step from a token loader
against the image path, and the three scripts end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

CODES6 = (70001, 70002, 70003, 70004, 70005, 70006)       # six different values above every code: a swapped pad / eos shows
STREAMS = ("coarse_content", "fine_content", "coarse_position", "fine_position")
SHAPES = [(4, 2), (8, 2), (12, 2), (16, 2), (8, 4)]
_ORACLE = {}


def grain_maps(hw1, seed):
    """B = 7: all coarse, all fine, one fine cell at cell 0, one at the last cell, checkerboard, one full fine cell-row, Bernoulli(0.5)"""
    g = np.zeros((7, hw1, hw1), dtype=np.int64)
    g[1] = 1
    g[2, 0, 0] = 1
    g[3, hw1 - 1, hw1 - 1] = 1
    g[4] = np.indices((hw1, hw1)).sum(0) % 2
    g[5, hw1 // 2] = 1
    g[6] = np.random.default_rng(seed).random((hw1, hw1)) < 0.5
    return g


def case(hw1, hw2, order, k):
    """(indices, grain, oracle streams) of one kernel case, computed once and shared"""
    from oracle import permuter as OP
    key = (hw1, hw2, order, k)
    if key not in _ORACLE:
        fhw = hw1 * hw2
        idx = np.random.default_rng(hw1 * 100 + hw2 + k).integers(0, k, size=(7, fhw, fhw))
        idx[0, 0, 0], idx[1, fhw - 1, fhw - 1] = k - 1, k - 1
        grain = grain_maps(hw1, seed=hw1 + hw2)
        want = OP.forward(idx, grain, hw1, hw2, order, *CODES6)
        for v in want.values():
            v.setflags(write=False)
        _ORACLE[key] = (idx, grain, want)
    return _ORACLE[key]


def pack_unpack(dev, idx, grain, hw1, hw2, order, k, extra=0, out=None):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import tokens as T
    codes, bits, n_fine, bad = K.tokens_pack(torch.from_numpy(idx).to(dev), torch.from_numpy(grain).to(dev), k)
    n = grain.reshape(grain.shape[0], -1).sum(1)
    assert bad.cpu().tolist() == [0] * idx.shape[0] and n_fine.cpu().tolist() == n.tolist()
    assert np.array_equal(bits.cpu().numpy(), T.pack_grain_bits(grain))                     # the ballot bitmap == the host's packbits
    assert np.array_equal(codes.cpu().numpy().astype(np.int64), idx.reshape(idx.shape[0], -1))
    lc, lf = T.row_lengths(n, hw1, hw2)
    return K.tokens_unpack(codes, bits, hw1, hw2, order, CODES6, lc + extra, lf + extra, n, out=out), (lc, lf)


@pytest.mark.parametrize("k", [1024, 65536])
@pytest.mark.parametrize("order", ["region-first", "row-first"])
@pytest.mark.parametrize("hw1,hw2", SHAPES)
def test_unpack_of_pack_equals_the_permuter(dev, hw1, hw2, order, k):
    from dynamicvectorquantization_amd._lib import DvqError
    from dynamicvectorquantization_amd.stage2 import DualGrainSeperatePermuter
    idx, grain, want = case(hw1, hw2, order, k)
    got, _ = pack_unpack(dev, idx, grain, hw1, hw2, order, k)
    for s in STREAMS:
        assert got[s].dtype == torch.int64 and np.array_equal(got[s].cpu().numpy(), want[s]), s
    for s, v in (("coarse_segment", 0), ("fine_segment", 1)):
        assert got[s].shape == got[s.replace("segment", "content")].shape and bool((got[s] == v).all())
    perm = DualGrainSeperatePermuter(hw1, hw1 * hw2, *CODES6, fine_position_order=order)
    args = dict(indices=torch.from_numpy(idx).to(dev), grain_indices=torch.from_numpy(grain).to(dev))
    if order == "row-first" and hw2 != 2:
        with pytest.raises(DvqError):            # dvq_permute_dual's row-first form stops at hw2 == 2; the closed form does not
            perm(**args)
        return
    mine = perm(**args)
    for s in STREAMS + ("coarse_segment", "fine_segment"):
        assert torch.equal(got[s], mine[s]), s


def test_single_image_batch(dev):
    from oracle import permuter as OP
    idx, grain, _ = case(12, 2, "row-first", 1024)
    want = OP.forward(idx[6:], grain[6:], 12, 2, "row-first", *CODES6)
    got, _ = pack_unpack(dev, idx[6:], grain[6:], 12, 2, "row-first", 1024)
    for s in STREAMS:
        assert np.array_equal(got[s].cpu().numpy(), want[s]), s


@pytest.mark.parametrize("order", ["region-first", "row-first"])
def test_longer_rows_hold_pad_codes(dev, order):
    idx, grain, want = case(12, 2, order, 1024)
    got, (lc, lf) = pack_unpack(dev, idx, grain, 12, 2, order, 1024, extra=5)
    pads = {"coarse_content": CODES6[0], "fine_content": CODES6[0], "coarse_position": CODES6[2], "fine_position": CODES6[4]}
    for s in STREAMS:
        a, n = got[s].cpu().numpy(), (lc if s.startswith("coarse") else lf)
        assert a.shape == (7, n + 5) and np.array_equal(a[:, :n], want[s]) and (a[:, n:] == pads[s]).all(), s


@pytest.mark.parametrize("order", ["region-first", "row-first"])
def test_guard_regions_stay_intact(dev, order):
    """outputs allocated inside larger sentinel-filled buffers: nothing before or after them is written, by either kernel"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import tokens as T
    hw1, hw2, guard = 12, 2, 64
    idx, grain, want = case(hw1, hw2, order, 1024)
    b, npix, w = 7, (hw1 * hw2) ** 2, T.grain_words(hw1)

    def guarded(numel, dtype, sentinel):
        big = torch.full((numel + 2 * guard,), sentinel, dtype=torch.int64, device=dev).to(dtype)
        return big, big[guard:guard + numel]

    bufs = [guarded(b * npix, torch.uint16, 0xABCD), guarded(b * w, torch.uint32, 0xABCDEF01), guarded(b, torch.int32, -77),
            guarded(b, torch.int32, -77)]
    out = (bufs[0][1].view(b, npix), bufs[1][1].view(b, w), bufs[2][1], bufs[3][1])
    codes, bits, n_fine, bad = K.tokens_pack(torch.from_numpy(idx).to(dev), torch.from_numpy(grain).to(dev), 1024, out=out)
    for (big, _), sentinel in zip(bufs, (0xABCD, 0xABCDEF01, -77, -77)):
        edge = torch.cat([big[:guard], big[-guard:]]).to(torch.int64)
        assert bool((edge == sentinel).all())
    assert bad.cpu().tolist() == [0] * b
    n = grain.reshape(b, -1).sum(1)
    lc, lf = T.row_lengths(n, hw1, hw2)
    sb = [guarded(b * l, torch.int64, -99) for l in (lc, lc, lf, lf)]
    got = K.tokens_unpack(codes, bits, hw1, hw2, order, CODES6, lc, lf, n, out=tuple(v.view(b, -1) for _, v in sb))
    for big, _ in sb:
        assert bool((torch.cat([big[:guard], big[-guard:]]) == -99).all())
    for s in STREAMS:
        assert np.array_equal(got[s].cpu().numpy(), want[s]), s


def test_bad_inputs_are_counted_clamped_and_contained(dev):
    """one code = K, one code = -1, one grain value = 2: counted per image; codes clamped, the bad grain written as coarse; the other
    images of the batch pack to the same bits as when packed alone"""
    from dynamicvectorquantization_amd import kernels as K
    hw1, hw2, k = 8, 2, 1024
    idx, grain, _ = case(hw1, hw2, "region-first", k)
    idx, grain = idx.copy(), grain.copy()
    idx[1, 3, 5], idx[1, 0, 1] = k, -1
    idx[4, 15, 15] = k + 70000
    grain[6, 2, 3] = 2
    grain[6, 2, 4] = -1
    codes, bits, n_fine, bad = K.tokens_pack(torch.from_numpy(idx).to(dev), torch.from_numpy(grain).to(dev), k)
    assert bad.cpu().tolist() == [0, 2, 0, 0, 1, 0, 2]
    c = codes.cpu().numpy().reshape(7, 16, 16)
    assert c[1, 3, 5] == k - 1 and c[1, 0, 1] == 0 and c[4, 15, 15] == k - 1
    clean = grain.copy()
    clean[6, 2, 3] = clean[6, 2, 4] = 0
    from dynamicvectorquantization_amd import tokens as T
    assert np.array_equal(bits.cpu().numpy(), T.pack_grain_bits(clean)) and n_fine.cpu().tolist() == clean.reshape(7, -1).sum(1).tolist()
    for i in (0, 2, 3, 5):
        alone = K.tokens_pack(torch.from_numpy(idx[i:i + 1]).to(dev), torch.from_numpy(grain[i:i + 1]).to(dev), k)
        assert torch.equal(alone[0][0], codes[i]) and torch.equal(alone[1][0], bits[i]) and int(alone[2][0]) == int(n_fine[i])
        assert int(alone[3][0]) == 0
    # a codebook larger than uint16: codes >= 65536 are out of range whatever codebook_size says
    big = np.full((1, 16, 16), 65536, dtype=np.int64)
    _, _, _, bad = K.tokens_pack(torch.from_numpy(big).to(dev), torch.from_numpy(grain[:1]).to(dev), 1 << 20)
    assert int(bad[0]) == 256


def test_wrapper_errors(dev):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import tokens as T
    hw1, hw2 = 8, 2
    idx, grain, _ = case(hw1, hw2, "region-first", 1024)
    ti, tg = torch.from_numpy(idx).to(dev), torch.from_numpy(grain).to(dev)
    codes, bits, _, _ = K.tokens_pack(ti, tg, 1024)
    n = grain.reshape(7, -1).sum(1)
    lc, lf = T.row_lengths(n, hw1, hw2)
    calls = []
    _lib._launch_hook = calls.append
    try:
        for bad_lc, bad_lf in ((lc - 1, lf), (lc, lf - 1)):
            with pytest.raises(ValueError):
                K.tokens_unpack(codes, bits, hw1, hw2, "region-first", CODES6, bad_lc, bad_lf, n)
        with pytest.raises(TypeError):
            K.tokens_unpack(codes.to(torch.int32), bits, hw1, hw2, "region-first", CODES6, lc, lf, n)
        with pytest.raises(TypeError):
            K.tokens_unpack(codes, bits.to(torch.int64), hw1, hw2, "region-first", CODES6, lc, lf, n)
        with pytest.raises(TypeError):
            K.tokens_pack(ti.to(torch.int32), tg, 1024)
        with pytest.raises(TypeError):
            K.tokens_pack(ti, tg.float(), 1024)
        with pytest.raises(ValueError):
            K.tokens_unpack(codes, bits, hw1, hw2, "column-first", CODES6, lc, lf, n)
        with pytest.raises(_lib.DvqError):
            K.tokens_unpack(codes.cpu(), bits.cpu(), hw1, hw2, "region-first", CODES6, lc, lf, n)       # host tensors
        with pytest.raises(_lib.DvqError):
            K.tokens_unpack(codes.t().contiguous().t(), bits, hw1, hw2, "region-first", CODES6, lc, lf, n)     # not contiguous
        with pytest.raises(_lib.DvqError):
            K.tokens_unpack(codes[:, :-1].contiguous(), bits, hw1, hw2, "region-first", CODES6, lc, lf, n)     # wrong shape
        assert calls == []                                   # none of these reached the library
        # 33 x 33 = 1089 cells > the 1024 whose word prefixes fit: the library's shape error, through check()
        c33 = torch.zeros(1, 66 * 66, dtype=torch.uint16, device=dev)
        b33 = torch.zeros(1, T.grain_words(33), dtype=torch.uint32, device=dev)
        with pytest.raises(_lib.DvqError, match="dvq_tokens_unpack"):
            K.tokens_unpack(c33, b33, 33, 2, "region-first", CODES6, 1090, 1, [0])
        assert calls == ["dvq_tokens_unpack"]
    finally:
        _lib._launch_hook = None


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def golden_dualformer(dev, kind):
    """the small golden Dualformer and its ragged 3-image batch, built as tests/test_gpu_likelihood.py::golden_dualformer builds them"""
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


def write_token_set(model, path, image_batches, labels=None):
    """encode -> tokens_pack -> writer (tokens.tokenize_batches) for a list of image batches -> the opened dataset"""
    from dynamicvectorquantization_amd import tokens as T
    fs = model.first_stage_model
    writer = T.TokenShardWriter(path, model.hw1, model.hw2, fs.quantize.codebook.n_embed, ["center"], shard_size=4, compute_dtype="fp32",
                                fingerprint=T.first_stage_fingerprint(fs), dataset={"test": True})
    i, feed = 0, []
    for k, x in enumerate(image_batches):
        b = int(x.shape[0])
        lab = labels[k] if labels is not None else np.full(b, -1)
        feed.append(([x], np.asarray(lab), np.arange(i, i + b)))
        i += b
    T.tokenize_batches(fs, feed, writer)
    writer.close()
    ds = T.TokenShardDataset(path, verify=True)
    ds.check_model(model)
    return ds


@pytest.mark.parametrize("kind", ["uncond", "class"])
def test_model_from_tokens_equals_model_from_images(dev, kind, tmp_path):
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import tokens as T
    with rt.compute_dtype_ctx(torch.float32):
        model, batch = golden_dualformer(dev, kind)
        model.eval()
        x, c = model.get_xc(batch)
        ds = write_token_set(model, str(tmp_path / "set"), [x], [batch["class_label"].cpu().numpy()])
        assert len(ds) == 3 and [f["records"] for f in ds.meta["files"]] == [3]
        loader = T.TokenBatchLoader(ds, 3, dev, model.permuter, shuffle=False)
        (tb,) = list(loader)
        torch.cuda.current_stream().synchronize()
        with torch.no_grad():
            _, z = model.encode_to_z(x)
        assert set(tb["tokens"]) == set(T.STREAM_KEYS) == set(z)
        for k in T.STREAM_KEYS:
            assert tb["tokens"][k].dtype == z[k].dtype and torch.equal(tb["tokens"][k], z[k]), k
        assert torch.equal(tb["class_label"], batch["class_label"])
        n_tok = [int((z["coarse_content"][i] < 512).sum() + (z["fine_content"][i] < 512).sum()) for i in range(3)]
        assert tb["n_tokens"] == n_tok and len(set(n_tok)) == 3                                         # the batch IS ragged
        tokens, tc = model.get_tc(tb)
        if kind == "uncond":
            assert "image" not in tb                                       # the conditioning never asks for the image that is not there
        # score
        model.train()
        flags = {n: m.training for n, m in model.named_modules()}
        st = model.score_tokens(tokens, tc)
        assert {n: m.training for n, m in model.named_modules()} == flags and model.transformer.training
        si = model.score(x, c)
        assert {n: m.training for n, m in model.named_modules()} == flags
        st, si = st.cpu().numpy(), si.cpu().numpy()
        print(kind, "score_tokens vs score: worst relative nll-sum difference", float(np.abs(st[:, :, 0] / si[:, :, 0] - 1).max()))
        assert st.shape == (3, 4, 4) and np.array_equal(st[:, :, 1:], si[:, :, 1:])
        np.testing.assert_allclose(st[:, :, 0], si[:, :, 0], rtol=1e-5)
        # with-loss forward, eval mode
        model.eval()
        with torch.no_grad():
            ft, fi = model.forward_tokens(tokens, tc), model(x, c)
        for k in ("content_loss", "position_loss", "coarse_position_loss", "fine_position_loss"):
            print(kind, k, float(ft[k]), float(fi[k]))
            np.testing.assert_allclose(float(ft[k]), float(fi[k]), rtol=1e-5)
        # shared_step takes the token path on a token batch, evaluate_likelihood accepts token batches
        with torch.no_grad():
            sh = model.shared_step(tb, 0)
        np.testing.assert_allclose(float(sh["content_loss"]), float(ft["content_loss"]), rtol=1e-5)
        s_tok = E.evaluate_likelihood(model, [tb], per_image=True)
        s_img = E.evaluate_likelihood(model, [batch], per_image=True)
    assert s_tok["pixels_per_image"] == s_img["pixels_per_image"] == 64 * 64 * 3 and s_tok["n_images"] == 3
    np.testing.assert_allclose(s_tok["per_image"][:, :, 0], s_img["per_image"][:, :, 0], rtol=1e-5)
    assert np.array_equal(s_tok["per_image"][:, :, 1:], s_img["per_image"][:, :, 1:])


def two_training_steps(dev, path, tmp_path):
    """two Trainer steps (fp32, dropout 0, AdamW at TRAIN_STEP_S2's rates without warm-up) of the golden uncond Dualformer on the two ragged
    batches of golden_cfg.train_step_s2_batch, fed as images or from a token set of the same images -> (logged scalars per step, strided
    sample of every transformer parameter, number of parameters that moved)"""
    from dynamicvectorquantization_amd import tokens as T
    from dynamicvectorquantization_amd.trainer import Trainer
    from golden_cfg import TRAIN_STEP_S2, train_step_s2_batch, train_step_stride
    c = TRAIN_STEP_S2
    images = [torch.from_numpy(train_step_s2_batch(s)).to(dev) for s in range(2)]
    model, _ = golden_dualformer(dev, "uncond")
    model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
    model.steps_per_epoch, model.training_steps = c["steps_per_epoch"], c["training_steps"]
    if path == "tokens":
        ds = write_token_set(model, str(tmp_path / "set"), images)
        feed = iter(T.TokenBatchLoader(ds, 3, dev, model.permuter, shuffle=False))
    else:
        feed = iter({"image": x} for x in images)
    model.train()
    start = {n: p.detach().clone() for n, p in model.transformer.named_parameters()}
    tr = Trainer(model, max_steps=2, use_graph=False)
    logs = []
    for step in range(2):
        tr.train_step(next(feed), step)
        logs.append({k: float(v) for k, v in model._logged.items()})
    params = {n: p.detach().reshape(-1)[::train_step_stride(p.numel())].double().cpu().numpy()
              for n, p in model.transformer.named_parameters()}
    moved = sum(int(not torch.equal(start[n], p.detach())) for n, p in model.transformer.named_parameters())
    return logs, params, moved


def parameter_distance(pa, pb, names):
    """worst relative L2 difference over the strided samples of the parameters `names`, and the parameter it belongs to"""
    return max((float(np.linalg.norm(pa[n] - pb[n]) / np.linalg.norm(pb[n])), n) for n in names)


# The attention KEY biases have an exactly zero gradient (a constant added to every key shifts each softmax row's logits equally); their
# fp32 gradient is rounding noise whose sign Adam turns into a full +-lr move (tests/golden_cfg.py says the same of the pinned step, which
# does not watch them).  Two runs of the IMAGE path differ there by up to 2.7e-4 (MI355X, worst of the 10 pairs of 5 runs, this very
# measure; docs/design/16-token-shards.md) and tokens against images by 1.7e-4 .. 2.9e-4: the bound for them is 4 x the image path's
# own spread.  Every other parameter keeps 1e-4.
PARAM_BOUND = 1e-4
KEY_BIAS_BOUND = 4 * 2.7e-4


def test_two_training_steps_from_tokens_equal_two_from_images(dev, tmp_path):
    """losses 1e-5 relative; a strided sample of every updated transformer parameter 1e-4 relative (L2 over the sample; the zero-gradient
    key biases: 4 x the spread of two image-path runs) -- the same kernels on bit-equal inputs, apart from the order of fp32 atomic folds"""
    from dynamicvectorquantization_amd import runtime as rt
    with rt.compute_dtype_ctx(torch.float32):
        li, pi, mi = two_training_steps(dev, "images", tmp_path)
        lt, pt, mt = two_training_steps(dev, "tokens", tmp_path)
    assert mi == mt == len(pi) and len(pi) > 20                                                  # every transformer parameter moved
    for step in range(2):
        assert set(li[step]) == set(lt[step]) and "train_loss" in li[step]
        for k in li[step]:
            print("step", step, k, lt[step][k], li[step][k])
            np.testing.assert_allclose(lt[step][k], li[step][k], rtol=1e-5)
    key_bias = [n for n in pi if n.endswith(".attn.key.bias")]
    rest = [n for n in pi if n not in key_bias]
    assert len(key_bias) == 4 and len(rest) > 20
    worst, name = parameter_distance(pt, pi, rest)
    worst_kb, name_kb = parameter_distance(pt, pi, key_bias)
    print("worst relative L2 parameter difference, tokens vs images:", worst, name, "| key biases:", worst_kb, name_kb)
    assert worst <= PARAM_BOUND, (worst, name)
    assert worst_kb <= KEY_BIAS_BOUND, (worst_kb, name_kb)


# ---- scripts -------------------------------------------------------------------------------------------------------------------------
def run_script(args, **kw):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=600, cwd=REPO, **kw)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_scripts_end_to_end(dev, tmp_path):
    """tokenize_dataset.py -> eval_likelihood.py --tokens (== --synthetic on images, view 0) -> train.py --token_data, each in a fresh
    process, on the tiny stage-2 config of tests/test_gpu_stage2.py with a saved first stage (every process must build the SAME one:
    check_model compares fingerprints)"""
    import yaml
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from test_gpu_stage2 import dualformer_config
    mc = dualformer_config()
    torch.manual_seed(5)
    fs = instantiate_from_config(mc["params"]["first_stage_config"])
    torch.save({"state_dict": fs.state_dict()}, tmp_path / "stage1.ckpt")
    mc["params"]["first_stage_config"]["params"]["ckpt_path"] = str(tmp_path / "stage1.ckpt")
    mc["base_learning_rate"] = 1e-5
    cfg = tmp_path / "tiny_stage2.yml"
    cfg.write_text(yaml.safe_dump({"model": mc, "data": {"target": "data.build.DataModuleFromConfig", "params": {"batch_size": 2}}}))
    out = tmp_path / "tokens"
    tool = os.path.join(REPO, "scripts/tools")
    r = run_script([os.path.join(tool, "tokenize_dataset.py"), "--yaml_path", str(cfg), "--synthetic", "6", "--views", "center,flip",
                    "--shard_size", "4", "--batch_size", "2", "--dtype", "fp32", "--out", str(out)])
    s = json.loads(r.stdout.strip().splitlines()[-1])
    assert s["images"] == 6 and s["views"] == 2 and s["records"] == 12 and s["images_per_s"] > 0
    assert s["tokens_per_image"] == {"mean": 40.0, "min": 40, "max": 40} and s["fine_ratio"] == 0.5     # half-flat: 8 coarse + 32 fine codes
    assert sorted(os.listdir(out)) == ["meta.json", "tokens-00000.npy", "tokens-00001.npy", "tokens-00002.npy"]
    meta = json.loads((out / "meta.json").read_text())
    assert [f["records"] for f in meta["files"]] == [4, 4, 4] and meta["views"] == ["center", "flip"] and meta["compute_dtype"] == "fp32"
    rec = np.load(out / "tokens-00000.npy", mmap_mode="r")
    assert rec["view"].tolist() == [0, 1, 0, 1] and rec["source"].tolist() == [0, 0, 1, 1] and rec["label"].tolist() == [-1] * 4
    assert not np.array_equal(rec["codes"][1], rec["codes"][0][:, ::-1])         # the flip view was encoded, not mirrored afterwards

    ev = os.path.join(tool, "eval_likelihood.py")
    common = ["--yaml_path", str(cfg), "--batch_size", "2", "--dtype", "fp32"]
    rt_ = run_script([ev] + common + ["--tokens", str(out), "--per_image", str(tmp_path / "tok.npy")])
    ri = run_script([ev] + common + ["--synthetic", "6", "--per_image", str(tmp_path / "img.npy")])
    st, si = json.loads(rt_.stdout.strip().splitlines()[-1]), json.loads(ri.stdout.strip().splitlines()[-1])
    a, b = np.load(tmp_path / "tok.npy"), np.load(tmp_path / "img.npy")
    assert a.shape == b.shape == (6, 4, 4) and np.array_equal(a[:, :, 1:], b[:, :, 1:])
    np.testing.assert_allclose(a[:, :, 0], b[:, :, 0], rtol=1e-5)
    assert set(st) == set(si) and st["n_images"] == 6 and st["pixels_per_image"] == si["pixels_per_image"] == 64 * 64 * 3
    for k in ("nats_per_image", "bits_per_image", "bits_per_pixel"):
        np.testing.assert_allclose(st[k], si[k], rtol=1e-5)
    for name in st["streams"]:
        for k, v in st["streams"][name].items():
            if k in ("tokens", "tokens_per_image", "top1", "top5"):
                assert v == si["streams"][name][k], (name, k)
            else:
                np.testing.assert_allclose(v, si["streams"][name][k], rtol=1e-5)
    r1 = run_script([ev] + common + ["--tokens", str(out), "--view", "1"])
    assert json.loads(r1.stdout.strip().splitlines()[-1])["nats_per_image"] != st["nats_per_image"]

    logs = tmp_path / "logs"
    run_script([os.path.join(REPO, "train.py"), "-b", str(cfg), "--token_data", str(out), "--token_val", str(out), "--max_steps", "3",
                "--precision", "fp32", "--logdir", str(logs), "-n", "t"])
    (run,) = os.listdir(logs)
    ck = torch.load(logs / run / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and any(k.startswith("transformer.") for k in ck["state_dict"])
