"""MaskVectorQuantize (the gradient-trained codebook) without a GPU: registration, constructor and state-dict layout as in the
reference, and tests/maskvq_math.py -- the torch-CPU restatement the GPU tests lean on -- reproducing every case of
tests/golden/maskvq.npz (reference outputs, tools/gen_golden_maskvq.py)."""
import glob
import os

import numpy as np
import pytest
import torch

import maskvq_math as M
from conftest import REPO, load_golden
from dynamicvectorquantization_amd import config

TARGET = "modules.vector_quantization.quantize_codebook_mask.MaskVectorQuantize"
YAML = "configs/stage1/dqvae-entropy-dual-r05-trainedcb_imagenet.yml"
TOL = 1e-6


def test_alias_resolves_and_yaml_loads():
    from dynamicvectorquantization_amd.quantize_trained import MaskVectorQuantize
    assert config.get_obj_from_str(TARGET) is MaskVectorQuantize
    config.install_reference_aliases()
    from modules.vector_quantization.quantize_codebook_mask import MaskVectorQuantize as aliased
    assert aliased is MaskVectorQuantize
    c = config.load_yaml(os.path.join(REPO, YAML))
    vq = c.model.params.vqconfig
    assert vq.target == TARGET
    assert dict(vq.params) == dict(codebook_size=1024, codebook_dim=256, accept_image_fmap=True, commitment_beta=0.25,
                                   use_cosine_sim=False, kmeans_init=False, orthogonal_reg_weight=0)
    q = config.instantiate_from_config(vq)
    assert isinstance(q, MaskVectorQuantize) and tuple(q.embedding.weight.shape) == (1024, 256)
    # everything but the quantiser is the EMA YAML
    ema = config.load_yaml(os.path.join(REPO, config.STAGE1_DUAL_ENTROPY_YAML))
    a, b = config.to_plain(c), config.to_plain(ema)
    a["model"]["params"].pop("vqconfig"), b["model"]["params"].pop("vqconfig")
    assert a == b


@pytest.mark.parametrize("kmeans_init", [False, True])
def test_state_dict_layout_and_initial_values(kmeans_init):
    q = config.get_obj_from_str(TARGET)(32, 8, kmeans_init=kmeans_init)
    sd = q.state_dict()
    assert list(sd.keys()) == ["initted", "cluster_size", "embedding.weight"]          # the reference's order
    assert [tuple(v.shape) for v in sd.values()] == [(1,), (1, 32), (32, 8)]
    assert sd["initted"].dtype == torch.float32 and float(sd["initted"]) == float(not kmeans_init)
    assert float(sd["cluster_size"].abs().max()) == 0.0
    w = sd["embedding.weight"]
    if kmeans_init:
        assert float(w.abs().max()) == 0.0
    else:
        assert 0.0 < float(w.abs().max()) <= 1.0 / 32 and float(w.min()) < 0 < float(w.max())       # U(+-1/K)
        assert abs(float(w.abs().mean()) * 32 - 0.5) < 0.1
    assert [n for n, _ in q.named_parameters()] == ["embedding.weight"] and q.embedding.weight.requires_grad
    assert q.is_initted() == (not kmeans_init)
    # a reference-layout state dict loads strictly
    ref = {"initted": torch.ones(1), "cluster_size": torch.full((1, 32), 3.0), "embedding.weight": torch.randn(32, 8)}
    q.load_state_dict(ref, strict=True)
    assert q.is_initted() and torch.equal(q.embedding.weight.detach(), ref["embedding.weight"])


def test_constructor_defaults_and_unknown_kwargs():
    cls = config.get_obj_from_str(TARGET)
    q = cls(16, 4)
    assert (q.kmeans_iters, q.use_cosine_sim, q.channel_last, q.accept_image_fmap, q.beta, q.orthogonal_reg_weight,
            q.activate_mask_quantize) == (10, False, False, True, 0.25, 0., True)
    for bad in (dict(decay=0.99), dict(restart_unused_codes=True), dict(use_ddp=False)):
        with pytest.raises(TypeError):
            cls(16, 4, **bad)
    with pytest.raises(NotImplementedError):
        cls(16, 4, accept_image_fmap=False)


def test_shipped_ema_yamls_still_build_vectorquantize2():
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, codebook_of
    paths = sorted(glob.glob(os.path.join(REPO, "configs", "stage1", "*.yml")))
    assert len(paths) >= 4
    for p in paths:
        vq = config.load_yaml(p).model.params.vqconfig
        if os.path.basename(p) == os.path.basename(YAML):
            continue
        params = dict(vq.params)
        params.update(codebook_size=16, codebook_dim=4)
        q = config.get_obj_from_str(vq.target)(**params)
        assert isinstance(q, VectorQuantize2), p
        w, k = codebook_of(q)
        assert w is q.codebook.weight and k == 16 and tuple(w.shape) == (17, 4)
    w, k = codebook_of(config.get_obj_from_str(TARGET)(16, 4))
    assert k == 16 and tuple(w.shape) == (16, 4)
    with pytest.raises(TypeError):
        codebook_of(torch.nn.Identity())


def test_model_passes_its_sampling_temperature_to_quantisers_that_take_one():
    """ae_fwd hands quant_sample_temperature to fwd() of a quantiser with `takes_temperature` and calls VectorQuantize2 as before
    (the GPU model test checks that a positive temperature really moves codes)"""
    import types
    from dynamicvectorquantization_amd import dqvae
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    assert config.get_obj_from_str(TARGET).takes_temperature is True
    assert not getattr(VectorQuantize2(16, 4), "takes_temperature", False)
    seen = []

    class Stop(Exception):
        pass

    def fwd_t(h, mask, tape, temp=None):
        seen.append(("t", temp))
        raise Stop

    def fwd_plain(h, mask, tape):
        seen.append(("plain",))
        raise Stop
    ns = types.SimpleNamespace
    for q in (ns(takes_temperature=True, fwd=fwd_t), ns(fwd=fwd_plain)):
        m = ns(feature_routed=True, quant_sample_temperature=0.7, quantize=q,
               encoder=ns(fwd=lambda x, g, t: (None, None, ns(indices=None, gate=torch.zeros(1)))), quant_conv=ns(fwd=lambda h, t: h))
        with pytest.raises(Stop):
            dqvae.DualGrainVQModel.ae_fwd(m, None, None)
    assert seen == [("t", 0.7), ("plain",)]


def test_replaced_pack_tables_stay_alive():
    """a recorded training step bakes the device address of its model's multi-tensor pack table into a launch; the convolutions of a
    SECOND model registering later must not free it (layers._PackRegistry.retired) -- two recorded Trainers in one process"""
    import gc
    import weakref
    from dynamicvectorquantization_amd.layers import LINEAR_PACKS, PACKS, Conv2d, Linear
    dev = torch.device("cpu")
    table = torch.zeros(16, dtype=torch.uint8)
    ref = weakref.ref(table)
    PACKS.tables[(torch.bfloat16, dev, 12345)] = {"sig": (), "table": table, "n": 0, "total": 0}
    del table
    Conv2d(8, 8, 3, padding=1)._alloc_pack(torch.bfloat16)          # another model's convolution registers its packed buffers
    gc.collect()
    assert (torch.bfloat16, dev, 12345) not in PACKS.tables and ref() is not None
    lt = torch.zeros(16, dtype=torch.uint8)
    lref = weakref.ref(lt)
    LINEAR_PACKS.tables[(dev, 12345)] = {"sig": (), "table": lt, "n": 0, "tiles": 0}
    del lt
    LINEAR_PACKS.register(Linear(8, 8))
    gc.collect()
    assert (dev, 12345) not in LINEAR_PACKS.tables and lref() is not None


# ---- the fixture against the formulas ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return load_golden("maskvq")


def test_golden_holds_fp32_and_int64_only(gold):
    for key in gold.files:
        assert gold[key].dtype in (np.float32, np.int64), key
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "maskvq.npz")) < 1_000_000


@pytest.mark.parametrize("case", range(len(M.SEARCH_SHAPES)))
def test_math_reproduces_search_cases(gold, case):
    shape = M.SEARCH_SHAPES[case]
    x, e = M.search_inputs(shape, int(gold[f"search{case}_seed"]))
    for name, cosine in (("l2", False), ("cos", True)):
        idx, _ = M.pick(M.scores(M.rows_of(x), e, cosine))
        ref = gold[f"search{case}_{name}_idx"]
        assert ref.shape == (shape[0], shape[2], shape[3])
        assert np.array_equal(idx.numpy(), ref.reshape(-1)), (shape, name)


@pytest.mark.parametrize("tag", list(M.MODULE_VARIANTS))
def test_math_reproduces_module_cases(gold, tag):
    cosine, with_mask, activate = M.MODULE_VARIANTS[tag]
    x, e, mask, g = M.module_inputs(tag, M.MODULE_SHAPE, int(gold[f"module_{tag}_seed"]))
    r = M.forward_backward(x, e, mask if with_mask else None, g, cosine=cosine, activate_mask=activate)
    assert np.array_equal(r["idx"], gold[f"module_{tag}_idx"])
    assert abs(r["loss"] - float(gold[f"module_{tag}_loss"])) <= TOL * abs(float(gold[f"module_{tag}_loss"]))
    for key in ("x_q", "dx", "dE"):
        assert M.rel_to_max(r[key], gold[f"module_{tag}_{key}"]) <= TOL, (tag, key)
    # the closed forms of the gradients, as the kernels compute them
    rows, gr = M.rows_of(x).double(), M.rows_of(g).double()
    n, d = rows.shape
    m = M.rows_of(mask).double() if with_mask and activate else torch.ones(n, 1, dtype=torch.float64)
    ratio = 1.0 / float(m.mean())
    eidx = torch.from_numpy(e).double()[torch.from_numpy(r["idx"]).reshape(-1)]
    dx = gr + M.G_LOSS * ratio * 2.0 * M.BETA / (n * d) * m * (rows - eidx)
    de = torch.zeros(e.shape, dtype=torch.float64).index_add_(0, torch.from_numpy(r["idx"]).reshape(-1),
                                                              M.G_LOSS * ratio * 2.0 / (n * d) * m * (eidx - rows))
    assert M.rel_to_max(dx.numpy(), M.rows_of(gold[f"module_{tag}_dx"]).numpy()) <= TOL
    assert M.rel_to_max(de.numpy(), gold[f"module_{tag}_dE"]) <= TOL


def test_math_reproduces_ortho_case(gold):
    x, e, mask, g = M.module_inputs("ortho", M.ORTHO_SHAPE, int(gold["ortho_seed"]))
    r = M.forward_backward(x, e, mask, g, ortho_w=M.ORTHO_W)
    r0 = M.forward_backward(x, e, mask, g, ortho_w=0.0)
    assert np.array_equal(r["idx"], gold["ortho_idx"])
    assert abs(r["loss"] - float(gold["ortho_loss"])) <= TOL * abs(float(gold["ortho_loss"]))
    assert M.rel_to_max(r["dE"], gold["ortho_dE"]) <= TOL
    # the term alone is stored as a difference of two fp32 results: its own rounding (2^-24 of the totals) is part of the bar
    assert abs(r["ortho"] - float(gold["ortho_term"])) <= TOL * abs(float(gold["ortho_loss"]))
    assert float(np.abs((r["dE"] - r0["dE"]) - gold["ortho_term_dE"]).max()) <= TOL * float(np.abs(gold["ortho_dE"]).max())


def test_math_reproduces_kmeans_case(gold):
    b, d, h, w, k = M.KMEANS_SHAPE
    x, perm = M.kmeans_inputs(int(gold["kmeans_seed"]))
    means, bins, hist = M.kmeans(M.rows_of(x), perm, k, M.KMEANS_ITERS)
    assert hist.shape == (M.KMEANS_ITERS, b * h * w)
    assert np.array_equal(bins, gold["kmeans_cluster_size"].reshape(-1))
    assert M.rel_to_max(means, gold["kmeans_weight"]) <= TOL
    assert (bins == 0).any(), "the case is meant to hold an empty cluster (it keeps its starting row)"
    idx, _ = M.pick(M.scores(M.rows_of(x), gold["kmeans_weight"], False))
    assert np.array_equal(idx.numpy(), gold["kmeans_idx"].reshape(-1))


def test_math_reproduces_model_level_quantiser(gold):
    """the quantiser inside the shrunken DQ-VAE: codes and qloss from the stored quantiser input and mask"""
    from dynamicvectorquantization_amd import synth
    k, zc = synth.DQVAE_GEOM["small"]["k"], synth.DQVAE_GEOM["small"]["zc"]
    e = (synth.det_param("quantize.codebook.weight.spread", (k + 1, zc)) * np.sqrt(zc) * 1.2).astype(np.float32)[:k]
    h = gold["model_h"]
    r = M.forward_backward(h, e, gold["model_mask"], np.zeros_like(h))
    assert np.array_equal(r["idx"], gold["model_codes"])
    assert abs(r["loss"] - float(gold["model_qloss"])) <= TOL * abs(float(gold["model_qloss"]))
