"""Image logging on the GPU (csrc/imagelog.hip, imagelog.py, the models' log_images, Trainer.fit(image_logger=...)).  `pytest -m gpu`.

The three kernels are compared with tests/imagelog_cpu.py -- the numpy restatement that tests/test_imagelog_cpu.py pins to the
reference's own draw functions -- and with the recorded fixture.  Equality is exact everywhere: every operation is specified in fp32
and the reductions are minima / maxima, so there is nothing to tolerate; a differing byte means contracted arithmetic or a reciprocal
multiply in the kernel."""
import os

import numpy as np
import pytest
import torch

import imagelog_cpu as IC
from conftest import REPO, load_golden
from dynamicvectorquantization_amd import synth

pytestmark = pytest.mark.gpu
F = np.float32
THRESHOLDS = os.path.join(REPO, "scripts/tools/thresholds/entropy_thresholds_imagenet_train_patch-16.json")


@pytest.fixture(scope="module")
def gold():
    return load_golden("imagelog")


def K():
    from dynamicvectorquantization_amd import kernels
    return kernels


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def as_bytes(a):
    k = np.rint(a * 255.0).astype(np.uint8)
    assert np.array_equal(k.astype(F) / F(255), a), "a colour panel is not k / 255"
    return k


def same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} values differ"


# ---- the three kernels ------------------------------------------------------------------------------------------------------------------
def test_overlay_and_lines_on_the_reference_fixture(dev, gold):
    """[2,3,256,256] with 16 x 16 (dual) / 8 x 8 (triple) maps and a score map: the reference's recorded bytes"""
    from dynamicvectorquantization_amd import imagelog as IL
    B = IC.FIXTURE_BATCH
    x = IC.fixture_images()
    g2, g3, sc = IC.fixture_grain(B, 16, 16, 2), IC.fixture_grain(B, 8, 8, 3), IC.fixture_score(B, 16, 16)
    xd = dv(x, dev)
    for key, kw_dev, kw_cpu in (("dual_color", dict(grain=dv(g2, dev), levels=2, scaler=0.7), dict(grain=g2, levels=2, scaler=0.7)),
                                ("triple_color", dict(grain=dv(g3, dev), levels=3, scaler=0.9), dict(grain=g3, levels=3, scaler=0.9)),
                                ("score_color", dict(score=dv(sc, dev), scaler=0.7), dict(score=sc, scaler=0.7))):
        got = K().grain_overlay(xd, **kw_dev).cpu().numpy()
        same(got, IC.overlay(x, **kw_cpu), key + " vs restatement")
        same(as_bytes(got), gold[key], key + " vs reference")
    same(xd, x, "the overlay's input")
    # the reference's names and defaults
    same(as_bytes(IL.draw_dual_grain_256res_color(images=xd.clone(), indices=dv(g2, dev), scaler=0.7).cpu().numpy()), gold["dual_color"], "draw dual")
    same(as_bytes(IL.draw_triple_grain_256res_color(images=xd.clone(), indices=dv(g3, dev)).cpu().numpy()), gold["triple_color"], "draw triple")
    same(as_bytes(IL.draw_dual_grain_256res_color(images=xd.clone(), indices=dv(sc, dev), scaler=0.7).cpu().numpy()), gold["score_color"], "draw score")
    for fn, g, lv, key in ((IL.draw_dual_grain_256res, g2, 2, "dual_lines"), (IL.draw_triple_grain_256res, g3, 3, "triple_lines")):
        ones = fn(indices=dv(g, dev)).cpu().numpy()                     # images=None: ones [B,3,256,256]
        assert ones.shape == (B, 3, 256, 256) and np.isin(ones, (1.0, -1.0)).all()
        for c in range(3):
            same((ones[:, c] == -1).astype(np.uint8), gold[key], f"{key} channel {c}")
        img = xd.clone()
        out = fn(images=img, indices=dv(g, dev))
        assert out is img                                               # drawn into the argument, like the reference
        same(out, IC.lines(x, g, lv), key + " on images")


def small_cases():
    rng = np.random.default_rng(11)
    x64 = rng.standard_normal((3, 3, 64, 64)).astype(F)                  # not in [-1, 1]: the overlay normalises by the image's own range
    x64[1] = F(0.375)                                                    # a constant image: hi - lo < 1e-5, the floor path
    g_dual = np.stack([np.zeros((4, 4), np.int64), np.ones((4, 4), np.int64), rng.integers(0, 2, (4, 4))])
    x32 = rng.uniform(-1, 1, (2, 3, 32, 32)).astype(F)
    g_tri = rng.integers(0, 3, (2, 8, 8))                                # cell 4: size // 4 == 1, quarter lines touch the borders
    g_tri[0, 0, :3] = (0, 1, 2)
    sc = (rng.integers(0, 257, (3, 4, 4)).astype(F) / F(256)).astype(F)
    sc[:, 0, 0], sc[:, 1, 1], sc[:, 2, 2] = 0.0, 1.0, 0.5
    return x64, g_dual.astype(np.int64), x32, g_tri.astype(np.int64), sc


def test_overlay_and_lines_small_shapes(dev):
    x64, g_dual, x32, g_tri, sc = small_cases()
    for scaler in (0.7, 0.9, 0.0, 1.0):
        same(K().grain_overlay(dv(x64, dev), grain=dv(g_dual, dev), levels=2, scaler=scaler),
             IC.overlay(x64, grain=g_dual, levels=2, scaler=scaler), f"dual 64 / 4x4 scaler {scaler}")
    same(K().grain_overlay(dv(x64, dev), grain=dv(g_dual, dev), levels=2, low=IC.RED, high=(0, 255, 0), scaler=0.7),
         IC.overlay(x64, grain=g_dual, levels=2, low=IC.RED, high=(0, 255, 0), scaler=0.7), "dual other colours")
    same(K().grain_overlay(dv(x32, dev), grain=dv(g_tri, dev), levels=3, scaler=0.9), IC.overlay(x32, grain=g_tri, levels=3, scaler=0.9),
         "triple 32 / 8x8")
    same(K().grain_overlay(dv(x64, dev), score=dv(sc, dev), scaler=0.7), IC.overlay(x64, score=sc, scaler=0.7), "score 64 / 4x4")
    # all-0 / all-1 dual maps paint exactly low / high: with scaler 1 the picture IS the colour
    full = K().grain_overlay(dv(x64, dev), grain=dv(g_dual, dev), levels=2, scaler=1.0).cpu().numpy()
    for b, col in ((0, IC.BLUE), (1, IC.RED)):
        for c in range(3):
            assert np.all(full[b, c] == F(col[c]) / F(255))
    # the constant image normalises to 0 everywhere: the blend of byte 0 towards the colour
    const = K().grain_overlay(dv(x64, dev), grain=dv(g_dual, dev), levels=2, scaler=0.7).cpu().numpy()[1]
    for c in range(3):
        assert np.all(const[c] == IC.blend_u8(np.uint8(0), np.uint8(IC.RED[c]), 0.7).astype(F) / F(255))
    for x, g, lv in ((x64, g_dual, 2), (x32, g_tri, 3), (x32, np.minimum(g_tri, 1), 2)):
        t = dv(x, dev)
        K().grain_lines_(t, dv(g, dev), lv)
        same(t, IC.lines(x, g, lv), f"lines {x.shape} levels {lv}")
    # a non-square image with square cells, more than one workgroup per image and a ragged last one
    xr = np.random.default_rng(5).uniform(-1, 1, (2, 3, 24, 36)).astype(F)
    gr = np.random.default_rng(6).integers(0, 3, (2, 2, 3)).astype(np.int64)
    same(K().grain_overlay(dv(xr, dev), grain=dv(gr, dev), levels=3, scaler=0.9), IC.overlay(xr, grain=gr, levels=3, scaler=0.9), "24 x 36")
    t = dv(xr, dev)
    K().grain_lines_(t, dv(gr, dev), 3)
    same(t, IC.lines(xr, gr, 3), "lines 24 x 36")


def test_shape_and_argument_errors(dev):
    from dynamicvectorquantization_amd._lib import DvqError
    x = torch.zeros(2, 3, 64, 64, device=dev)
    for h, w in ((5, 5), (4, 8), (3, 4)):                                # h does not divide H / unequal cells
        with pytest.raises(DvqError, match=r"code -2"):
            K().grain_overlay(x, grain=torch.zeros(2, h, w, dtype=torch.int64, device=dev))
        with pytest.raises(DvqError, match=r"code -2"):
            K().grain_lines_(x.clone(), torch.zeros(2, h, w, dtype=torch.int64, device=dev), 2)
    g = torch.zeros(2, 4, 4, dtype=torch.int64, device=dev)
    with pytest.raises(DvqError, match=r"code -1"):
        K().grain_overlay(x, grain=g, levels=4)
    with pytest.raises(DvqError, match=r"code -1"):
        K().grain_overlay(x, grain=g, scaler=1.5)
    with pytest.raises(DvqError, match=r"code -5"):
        K().grain_overlay(x, grain=g, ws=torch.empty(8, dtype=torch.uint8, device=dev))
    with pytest.raises(DvqError, match=r"code -2"):
        K().image_grid_u8(torch.zeros(2, 2, 8, 8, device=dev))
    with pytest.raises(DvqError, match=r"code -5"):
        K().image_grid_u8(torch.zeros(2, 3, 8, 8, device=dev), out=torch.empty(10, dtype=torch.uint8, device=dev))
    with pytest.raises(DvqError):
        K().grain_overlay(torch.zeros(2, 3, 64, 64), grain=g.cpu())      # no host path
    assert torch.equal(x, torch.zeros_like(x))


GRID_SHAPES = [(5, 3, 20, 12), (4, 3, 8, 8), (1, 3, 9, 7), (3, 1, 6, 10), (1, 1, 5, 5), (9, 3, 33, 17)]


@pytest.mark.parametrize("shape", GRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grid_against_restatement(dev, shape):
    """N = 5 (a second row with three empty cells), N = 4, N = 1 (no padding), C = 1, H != W; values outside [-1, 1], clamp on and off"""
    rng = np.random.default_rng(sum(shape))
    v = (rng.integers(-300, 301, size=shape).astype(F) / F(200)).astype(F)
    for clamp in (True, False):
        for nrow, pad in ((4, 2), (3, 0), (8, 1)):
            got = K().image_grid_u8(dv(v, dev), nrow=nrow, padding=pad, clamp=clamp)
            assert tuple(got.shape[:2]) == IC.grid_shape(shape[0], shape[2], shape[3], nrow, pad) == \
                K().image_grid_shape(shape[0], shape[2], shape[3], nrow, pad)
            same(got, IC.grid_u8(v, nrow=nrow, padding=pad, clamp=clamp), f"grid {shape} nrow {nrow} padding {pad} clamp {clamp}")
    inside = np.clip(v, -1, 1)                                           # nothing to clamp: the flag changes nothing
    same(K().image_grid_u8(dv(inside, dev), clamp=True), K().image_grid_u8(dv(inside, dev), clamp=False).cpu().numpy(), "clamp flag")
    const = np.full(shape, -0.5, dtype=F)                                # hi - lo < 1e-5: the floor, all zero
    assert not K().image_grid_u8(dv(const, dev)).any()


def test_grid_on_the_recorded_fixture(dev, gold):
    for name in ("grid5", "grid1", "grid4_c1"):
        for clamp in (True, False):
            same(K().image_grid_u8(dv(gold[name + "_in"], dev), nrow=4, padding=2, clamp=clamp),
                 gold[f"{name}_{'clamp' if clamp else 'raw'}"], f"{name} clamp {clamp}")


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB")).copy()


def test_logger_keeps_the_first_max_images(dev, tmp_path):
    """max_images smaller than the batch: the grid holds the first of them and is normalised by their range alone; two keys, one
    event; file names of utils/logger.py:144"""
    from dynamicvectorquantization_amd.imagelog import ImageLogger
    rng = np.random.default_rng(2)
    v = rng.uniform(-1, 1, (6, 3, 10, 14)).astype(F)
    v[5] *= F(4)                                                        # outside the kept images
    m = rng.uniform(0, 1, (6, 1, 10, 14)).astype(F)
    lg = ImageLogger(str(tmp_path), batch_frequency=1, max_images=3, clamp=False)
    for step in range(4):                                               # more events than the queue holds: backpressure, not loss
        lg.log_local("val", {"a": dv(v, dev), "mask": dv(m, dev), "caption": ["x"] * 6}, 12 + step, 3, 7)
    lg.flush()
    root = os.path.join(str(tmp_path), "images", "val")
    assert sorted(os.listdir(root)) == sorted(f"Step_{12 + s:06}-Epoch_003-Batch_000007-{k}.png" for s in range(4) for k in ("a", "mask"))
    assert lg.written == [os.path.join(root, f"Step_{12 + s:06}-Epoch_003-Batch_000007-{k}.png") for s in range(4) for k in ("a", "mask")]
    for s in range(4):
        same(read_png(os.path.join(root, f"Step_{12 + s:06}-Epoch_003-Batch_000007-a.png")), IC.grid_u8(v[:3], clamp=False), "kept images")
        same(read_png(os.path.join(root, f"Step_{12 + s:06}-Epoch_003-Batch_000007-mask.png")), IC.grid_u8(m[:3], clamp=False), "C = 1")
    lg.flush()                                                          # idempotent


# ---- log_images on tiny models ----------------------------------------------------------------------------------------------------------
def tiny_stage1(kind, dev):
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config, stage1_config
    torch.manual_seed(0)
    if kind == "entropy":
        cfg = stage1_config(objective="ae", geometry=synth.DQVAE_GEOM["small"]).model
    else:
        from test_gpu_featrouted import feat_model_config
        cfg = feat_model_config(kind)
    model = instantiate_from_config(cfg).to(dev)
    rt.bump_weights_epoch()
    return model


@pytest.mark.parametrize("kind", ["entropy", "dualfeat", "triple"])
def test_log_images_stage1(dev, kind):
    from dynamicvectorquantization_amd import imagelog as IL
    from dynamicvectorquantization_amd import runtime as rt
    want_keys = {"entropy": ["inputs", "reconstructions", "grain_map", "entropy_map"],
                 "dualfeat": ["inputs", "reconstructions", "grain_color"],
                 "triple": ["inputs", "reconstructions", "grain", "grain_color"]}[kind]
    x = synth.half_flat_images(3, 64, seed=5)
    with rt.compute_dtype_ctx(torch.bfloat16):
        model = tiny_stage1(kind, dev).eval()
        batch = {"image": dv(x, dev)}
        log = model.log_images(batch)
        with torch.no_grad():
            out = model(batch["image"])
        grain = out[2].cpu().numpy()
        assert list(log) == want_keys
        for k, v in log.items():
            assert tuple(v.shape) == (3, 3, 64, 64) and v.dtype == torch.float32 and v.is_cuda, k
            assert bool(torch.isfinite(v).all()), k
        same(log["inputs"], x, "inputs")
        same(log["reconstructions"], out[0].cpu().numpy(), "reconstructions")           # the eval forward is repeatable
        levels = 3 if kind == "triple" else 2
        assert grain.shape[0] == 3 and set(np.unique(grain)) <= set(range(levels))
        if kind == "entropy":
            same(log["grain_map"], IC.overlay(x, grain=grain, levels=2, scaler=0.7), "grain_map")
            score = IL.normalize_scores(out[4])
            assert float(score.min()) == 0.0 and float(score.max()) == 1.0
            e = out[4].cpu().numpy()
            lo, hi = F(e.min()), F(e.max())
            np.testing.assert_allclose(score.cpu().numpy(), (e - lo) / max(F(hi - lo), F(1e-5)), rtol=3e-7, atol=0)  # torch's own division
            same(log["entropy_map"], IC.overlay(x, score=score.cpu().numpy(), scaler=0.7), "entropy_map")
        elif kind == "dualfeat":
            same(log["grain_color"], IC.overlay(x, grain=grain, levels=2, scaler=0.7), "grain_color")
        else:
            same(log["grain"], IC.lines(x, grain, 3), "grain")
            same(log["grain_color"], IC.overlay(x, grain=grain, levels=3, scaler=0.9), "grain_color")
        # max_images: fewer grain pictures, the same values
        part = model.log_images(batch, max_images=2)
        assert list(part) == want_keys
        for k in want_keys[2:]:
            same(part[k], log[k][:2].cpu().numpy(), k + " (max_images)")


@pytest.mark.parametrize("kind", ["uncond", "class"])
def test_log_images_stage2(dev, kind):
    """keys and their order, N = 4, finite pictures; inputs / reconstructions only during epoch 0; the draws come from the state the
    caller passes -- repeatable for a seed, different for another -- and leave the model's own sampler stream and torch's generators
    where they were"""
    from golden_cfg import dualformer_cfg
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    target = {"uncond": "models.stage2_dynamic.dqtransformer_uncond_entropy.Dualformer",
              "class": "models.stage2_dynamic.dqtransformer_class2_entropy.Dualformer"}[kind]
    with rt.compute_dtype_ctx(torch.bfloat16):
        torch.manual_seed(4)
        model = instantiate_from_config({"target": target, "params": dualformer_cfg(kind, json_path=THRESHOLDS)}).to(dev).eval()
        rt.bump_weights_epoch()
        batch = {"image": dv(synth.half_flat_images(6, 64, seed=9), dev)}
        if kind == "class":
            batch["class_label"] = torch.tensor([1, 4, 9, 0, 3, 7], device=dev)

        def state(seed):
            return torch.tensor([seed, 0], dtype=torch.int64, device=dev)

        # the model's own stream exists and has advanced before the log event
        c = model.encode_to_c(model.get_xc(batch, 2)[1])
        model.sample_from_scratch(*c, sample=True, top_k=20, top_k_pos=10, process=False)
        own = model.__dict__["_sampler_state"]
        own_before, cpu_rng, gpu_rng = own.clone(), torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        assert int(own_before[1]) > 0

        model.current_epoch = 0
        st = state(77)
        a = model.log_images(batch, sampler_state=st)
        assert list(a) == ["samples_fixed_fine_position", "samples_from_scratch", "inputs", "reconstructions"]
        for k, v in a.items():
            assert tuple(v.shape) == (4, 3, 64, 64) and v.dtype == torch.float32 and bool(torch.isfinite(v).all()), k
        same(a["inputs"], batch["image"][:4].cpu().numpy(), "inputs")
        assert int(st[0]) == 77 and int(st[1]) > 0                       # the passed state advanced ...
        assert model.__dict__["_sampler_state"] is own and torch.equal(own, own_before)     # ... the model's own did not
        assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(dev), gpu_rng)

        model.current_epoch = 1
        b = model.log_images(batch, sampler_state=state(77))
        assert list(b) == ["samples_fixed_fine_position", "samples_from_scratch"]
        other = model.log_images(batch, sampler_state=state(78))
        for k in b:
            same(b[k], a[k].cpu().numpy(), k + " repeats for the seed")
        assert any(not torch.equal(other[k], a[k]) for k in b), "another seed drew the same pictures"
        assert torch.equal(own, own_before)
        # a token batch (train.py --token_data) holds no images: the two sample panels only, also during epoch 0
        model.current_epoch = 0
        tok = {"tokens": model.encode_to_z(batch["image"])[1], **{k: v for k, v in batch.items() if k != "image"}}
        t = model.log_images(tok, sampler_state=state(77))
        assert list(t) == ["samples_fixed_fine_position", "samples_from_scratch"]
        for k in t:
            same(t[k], a[k].cpu().numpy(), k + " from a token batch")


# ---- around the training step -----------------------------------------------------------------------------------------------------------
def training_setup(dev, max_steps):
    from dynamicvectorquantization_amd.trainer import Trainer
    model = tiny_stage1("entropy", dev)
    model.learning_rate, model.training_steps, model.steps_per_epoch = 1e-4, 100, 100
    model.train()
    pool = [dv(synth.half_flat_images(4, 64, seed=20 + i), dev) for i in range(2)]
    return model, Trainer(model, max_steps=max_steps), (lambda step: {"image": pool[step % 2]})


def test_log_event_leaves_training_untouched(dev, tmp_path):
    """after >= 3 replays of the recorded step: every parameter, every buffer (the VQ's EMA statistics among them), the optimizer's
    moments, global_step and every submodule's training flag are bitwise what they were before the event, and the next step replays"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.imagelog import ImageLogger
    with rt.compute_dtype_ctx(torch.bfloat16):
        model, tr, batch_fn = training_setup(dev, 20)
        model.loss.eval()                                               # a submodule that is NOT in training mode must stay so
        for step in range(7):
            tr.train_step(batch_fn(step), step)
        assert tr.use_graph and tr.graph_replays >= 3, (tr.use_graph, tr.graph_replays)

        def snapshot():
            torch.cuda.synchronize()
            tensors = {"p:" + n: p.detach().clone() for n, p in model.named_parameters()}
            tensors.update({"b:" + n: b.detach().clone() for n, b in model.named_buffers()})
            for i, o in enumerate(tr.opts):
                tensors[f"m:{i}"], tensors[f"v:{i}"] = o._fstate["m"].clone(), o._fstate["v"].clone()
            flags = [(n, m.training) for n, m in model.named_modules()]
            host = (int(model.global_step), [o._fstate["step"] for o in tr.opts], [s["scheduler"].state_dict() for s in tr.scheds],
                    torch.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone())
            return tensors, flags, host

        before = snapshot()
        assert any(k.startswith("b:") and "ema" in k for k in before[0]), sorted(before[0])[:5]
        lg = ImageLogger(str(tmp_path), batch_frequency=1, max_images=16)
        replays = tr.graph_replays
        assert lg.maybe_log(model, batch_fn(7), 7, "train") is True
        after = snapshot()
        assert before[1] == after[1] and (False in [f for _, f in after[1]]) and (True in [f for _, f in after[1]])
        assert before[2][:2] == after[2][:2] and before[2][2] == after[2][2]
        assert torch.equal(before[2][3], after[2][3]) and torch.equal(before[2][4], after[2][4])
        assert set(before[0]) == set(after[0])
        for k in before[0]:
            assert torch.equal(before[0][k], after[0][k]), k
        losses = tr.train_step(batch_fn(7), 7)                          # the recorded step still applies
        assert tr.graph_replays == replays + 1 and all(bool(torch.isfinite(l).all()) for l in losses)
        assert int(model.global_step) == 8
        lg.flush()
        names = sorted(os.listdir(os.path.join(str(tmp_path), "images", "train")))
        assert names == sorted(f"Step_000007-Epoch_000-Batch_000007-{k}.png" for k in ("inputs", "reconstructions", "grain_map", "entropy_map"))


def test_fit_writes_the_expected_pictures(dev, tmp_path):
    """Trainer.fit for 5 steps, a picture every 2 batches: exactly the files of batches 0, 2, 4 for every key once fit has returned
    (it flushes); decoded pixels equal the grid kernel's bytes; without a logger nothing is written"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.imagelog import ImageLogger
    keys = ("inputs", "reconstructions", "grain_map", "entropy_map")
    with rt.compute_dtype_ctx(torch.bfloat16):
        model, tr, batch_fn = training_setup(dev, 5)
        lg = ImageLogger(str(tmp_path), batch_frequency=2, max_images=3)
        tr.fit(batch_fn, image_logger=lg)
        root = os.path.join(str(tmp_path), "images", "train")
        want = sorted(f"Step_{b + 1:06}-Epoch_000-Batch_{b:06}-{k}.png" for b in (0, 2, 4) for k in keys)
        assert sorted(os.listdir(root)) == want and os.listdir(str(tmp_path)) == ["images"] and lg.events == 3
        assert os.listdir(os.path.join(str(tmp_path), "images")) == ["train"]
        assert model.training and int(model.global_step) == 5
        # the weights have not moved since the event of batch 4: its panels again, through the grid kernel and the restatement
        model.eval()
        panels = model.log_images(batch_fn(4))
        model.train()
        for k in keys:
            png = read_png(os.path.join(root, f"Step_000005-Epoch_000-Batch_000004-{k}.png"))
            first = panels[k][:3].contiguous()
            same(png, K().image_grid_u8(first, nrow=4, padding=2, clamp=True).cpu().numpy(), k + " vs kernel")
            same(png, IC.grid_u8(first.cpu().numpy(), nrow=4, padding=2, clamp=True), k + " vs restatement")
            assert png.shape == (64 + 4, 3 * 66 + 2, 3)
        # logger absent: two more steps, nothing appears
        tr.max_steps = 7
        tr.fit(batch_fn)
        assert int(model.global_step) == 7 and sorted(os.listdir(root)) == want and os.listdir(str(tmp_path)) == ["images"]
        other = tmp_path / "none"
        other.mkdir()
        model2, tr2, batch_fn2 = training_setup(dev, 2)
        tr2.fit(batch_fn2, ckpt_path=str(other / "checkpoints" / "last.ckpt"))
        assert sorted(os.listdir(str(other))) == ["checkpoints"]
