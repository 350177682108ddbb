"""MaskVectorQuantize (the gradient-trained codebook) on the GPU: the search kernels (temp 0 and Gumbel), the noise law, the module's
forward / backward against the reference goldens (tests/golden/maskvq.npz, tools/gen_golden_maskvq.py), the codebook-gradient kernel,
the orthogonality term, the k-means initialisation, the shrunken DQ-VAE carrying this quantiser, and the evaluation / token-shard
helpers around it.  tests/maskvq_math.py is the fp64 restatement.  `pytest -m gpu`."""
import copy
import math

import numpy as np
import pytest
import torch

import maskvq_math as M
from conftest import load_golden
from dynamicvectorquantization_amd import synth

pytestmark = pytest.mark.gpu

TARGET = "modules.vector_quantization.quantize_codebook_mask.MaskVectorQuantize"
PARITY = 1e-3             # the project's parity bar: max error relative to the tensor's max-norm
BF16_ULP = 2.0 ** -8      # one unit in the last place of a bf16 value: what a tensor STORED in bf16 can be off by after its last rounding


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def gold():
    return load_golden("maskvq")


def make(dev, e, **kw):
    from dynamicvectorquantization_amd.config import get_obj_from_str
    k, d = e.shape
    q = get_obj_from_str(TARGET)(k, d, **kw).to(dev).eval()
    with torch.no_grad():
        q.embedding.weight.copy_(T(e, dev))
    return q


def nhwc(x, dev, dtype):
    return T(x, dev).permute(0, 2, 3, 1).contiguous().to(dtype)


# ---- 1. search, temp 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["fp32", "bf16"])
@pytest.mark.parametrize("metric", ["l2", "cos"])
@pytest.mark.parametrize("case", range(len(M.SEARCH_SHAPES)))
def test_search_temp0_matches_golden(dev, gold, case, metric, rows):
    shape = M.SEARCH_SHAPES[case]
    x, e = M.search_inputs(shape, int(gold[f"search{case}_seed"]))
    cosine = metric == "cos"
    q = make(dev, e, use_cosine_sim=cosine)
    dtype = torch.float32 if rows == "fp32" else torch.bfloat16
    _, _, idx = q.fwd(nhwc(x, dev, dtype), None, None)
    if rows == "fp32":
        ref = gold[f"search{case}_{metric}_idx"]
    else:      # the fp64 argmax on the bf16-rounded rows
        ref = M.pick(M.scores(M.bf16_round(M.rows_of(x)), e, cosine))[0].numpy().reshape(shape[0], shape[2], shape[3])
    got = idx.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.int64
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} indices differ"


@pytest.mark.parametrize("d", [64, 72])
def test_search_ties_and_zero_rows(dev, d):
    """duplicated code rows: the lower index wins, in the exact L2 search, the cosine search and the noiseless L2 form of the new kernel;
    an all-zero row under cosine scores 0 against every code: index 0"""
    from dynamicvectorquantization_amd import kernels as K
    r = M.rng(f"ties{d}")
    k, n = 70, 150
    e = r.standard_normal((k, d)).astype(np.float32)
    e[40] = e[3]
    e[69] = e[33]
    e[34] = e[33]
    x = r.standard_normal((n, d)).astype(np.float32)
    x[:50] = e[3] + 0.01 * r.standard_normal((50, d)).astype(np.float32)
    x[50:100] = 2.0 * e[33] + 0.01 * r.standard_normal((50, d)).astype(np.float32)
    x[120] = 0.0
    for cosine in (False, True):
        s64 = M.scores(x, e, cosine)
        s64[:, [34, 40, 69]] = -float("inf")          # a duplicate never beats its lower-indexed twin: the fp64 argmax without them
        ref = M.pick(s64)[0].numpy()
        assert set(ref[:50].tolist()) == {3} and set(ref[50:100].tolist()) == {33}
        q = make(dev, e, use_cosine_sim=cosine)
        _, _, idx = q.fwd(T(x, dev).view(1, 1, n, d), None, None)
        assert np.array_equal(idx.cpu().numpy().reshape(-1), ref), cosine
        prep = K.vq_trained_prepare(T(e, dev), cosine)
        assert np.array_equal(K.vq_sample_argmax(T(x, dev), prep, k, cosine, 0.0, codebook=T(e, dev)).cpu().numpy(), ref), cosine
        if cosine:
            assert ref[120] == 0


# ---- 2. Gumbel search -------------------------------------------------------------------------------------------------------------------
GUMBEL_CASES = [(192, 1024, 256, False, 20.0, "fp32"), (192, 1024, 256, False, 1.0, "fp32"), (256, 512, 64, True, 0.05, "fp32"),
                (100, 100, 72, False, 8.0, "fp32"), (4096, 1024, 256, False, 20.0, "bf16")]


@pytest.mark.parametrize("n,k,d,cosine,temp,rows", GUMBEL_CASES)
def test_gumbel_search_matches_fp64_with_regenerated_noise(dev, n, k, d, cosine, temp, rows):
    from dynamicvectorquantization_amd import kernels as K
    r = M.rng(f"gumbel{n},{k},{d}")
    x = r.standard_normal((n, d)).astype(np.float32)
    e = r.standard_normal((k, d)).astype(np.float32)
    xt = T(x, dev) if rows == "fp32" else T(x, dev).to(torch.bfloat16)
    x_eff = x if rows == "fp32" else M.bf16_round(x)
    prep = K.vq_trained_prepare(T(e, dev), cosine)
    state = torch.tensor([0x1234567 + n, 41], dtype=torch.int64, device=dev)
    seed, counter = (int(v) for v in state.cpu())
    idx = K.vq_sample_argmax(xt, prep, k, cosine, temp, state).cpu().numpy()
    assert [int(v) for v in state.cpu()] == [seed, counter + 1]          # exactly one draw per call
    noise = K.vq_gumbel_noise(seed, counter, n, k, dev).cpu().double()
    s64 = M.scores(x_eff, e, cosine)
    ref, gap = M.pick(s64, temp, noise)
    excl = (gap < 1e-5 * s64.abs().max(dim=1).values / temp).numpy()
    print(f"gumbel N{n} K{k} D{d} cos{int(cosine)} temp{temp} {rows}: excluded {int(excl.sum())}, "
          f"mismatches outside {int((idx != ref.numpy())[~excl].sum())}")
    assert excl.mean() <= 0.005
    assert np.array_equal(idx[~excl], ref.numpy()[~excl])
    if temp in (20.0, 0.05):
        moved = float((idx != M.pick(s64)[0].numpy()).mean())
        print(f"  moved off the noiseless argmax: {moved:.3f}")
        assert moved > 0.5
    # the same (seed, counter) reproduces the picks bit for bit, the next counter does not
    state.copy_(torch.tensor([seed, counter], dtype=torch.int64))
    assert np.array_equal(K.vq_sample_argmax(xt, prep, k, cosine, temp, state).cpu().numpy(), idx)
    assert not np.array_equal(K.vq_sample_argmax(xt, prep, k, cosine, temp, state).cpu().numpy(), idx)
    assert int(state.cpu()[1]) == counter + 2


# ---- 3. noise law ---------------------------------------------------------------------------------------------------------------------
def test_gumbel_noise_law(dev):
    from dynamicvectorquantization_amd import kernels as K
    g = K.vq_gumbel_noise(20240917, 5, 1024, 1024, dev).double()
    assert bool(torch.isfinite(g).all())
    mean, var = float(g.mean()), float(g.var())
    print(f"gumbel noise: mean {mean:.5f} (0.57722), variance {var:.5f} ({math.pi ** 2 / 6:.5f})")
    assert abs(mean - 0.5772156649) < 0.01
    assert abs(var - math.pi ** 2 / 6) < 0.03
    assert not torch.equal(g, K.vq_gumbel_noise(20240917, 6, 1024, 1024, dev).double())
    assert not torch.equal(g, K.vq_gumbel_noise(20240918, 5, 1024, 1024, dev).double())


def test_gumbel_pick_frequencies_follow_softmax(dev):
    """one row repeated 65 536 times against 8 codes: argmax(s / temp + g) is a draw from softmax(s / temp)"""
    from dynamicvectorquantization_amd import kernels as K
    r = M.rng("softmax")
    n, k, d = 65536, 8, 64
    row = r.standard_normal((1, d)).astype(np.float32)
    e = r.standard_normal((k, d)).astype(np.float32)
    s64 = M.scores(row, e, False)[0]
    temp = float(s64.std())                                   # spreads the softmax: the scores / temp have unit spread
    p = torch.softmax(s64 / temp, dim=0).numpy()
    assert p.min() > 0.005 and p.max() < 0.9, p
    state = torch.tensor([77, 0], dtype=torch.int64, device=dev)
    prep = K.vq_trained_prepare(T(e, dev), False)
    idx = K.vq_sample_argmax(T(np.repeat(row, n, axis=0), dev), prep, k, False, temp, state).cpu().numpy()
    counts = np.bincount(idx, minlength=k)
    sd = np.sqrt(n * p * (1 - p))
    print("pick frequencies: deviations in binomial standard deviations", np.round((counts - n * p) / sd, 2).tolist())
    assert np.all(np.abs(counts - n * p) <= 5 * sd)


# ---- 4. module forward / backward ---------------------------------------------------------------------------------------------------
def run_module(dev, q, x, mask, g):
    xt = T(x, dev).requires_grad_(True)
    q.embedding.weight.grad = None
    xq, loss, (_, _, idx) = q(xt, 0., codebook_mask=None if mask is None else T(mask, dev))
    ((xq * T(g, dev)).sum() + M.G_LOSS * loss).backward()
    return dict(x_q=xq.detach().cpu().numpy(), loss=float(loss.detach()), idx=idx.cpu().numpy(), dx=xt.grad.cpu().numpy(),
                dE=q.embedding.weight.grad.cpu().numpy())


@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
@pytest.mark.parametrize("tag", list(M.MODULE_VARIANTS))
def test_module_forward_backward_golden(dev, gold, tag, mode):
    from dynamicvectorquantization_amd import runtime as rt
    cosine, with_mask, activate = M.MODULE_VARIANTS[tag]
    x, e, mask, g = M.module_inputs(tag, M.MODULE_SHAPE, int(gold[f"module_{tag}_seed"]))
    with rt.compute_dtype_ctx(mode):
        q = make(dev, e, use_cosine_sim=cosine, activate_mask_quantize=activate)
        r = run_module(dev, q, x, mask if with_mask else None, g)
    assert np.array_equal(r["idx"], gold[f"module_{tag}_idx"])
    errs = {key: M.rel_to_max(r[key], gold[f"module_{tag}_{key}"]) for key in ("x_q", "dx", "dE")}
    errs["loss"] = abs(r["loss"] - float(gold[f"module_{tag}_loss"])) / abs(float(gold[f"module_{tag}_loss"]))
    print(f"module {tag} {mode}: relative-to-max errors {errs}")
    assert all(v < PARITY for v in errs.values()), errs


@pytest.mark.parametrize("tag", list(M.MODULE_VARIANTS))
def test_module_forward_backward_bf16(dev, gold, tag):
    """bf16 compute: the same case against the fp64 restatement evaluated on the bf16-rounded input (and upstream gradient).  Indices exact
    (as the existing bf16 VQ tests of test_gpu_kernels.py ask of the search: exact w.r.t. the bf16-rounded rows); the fp32 results (loss,
    codebook gradient) at the parity bar; x_q and dx are stored in bf16: one bf16 ulp of their max-norm"""
    from dynamicvectorquantization_amd import runtime as rt
    cosine, with_mask, activate = M.MODULE_VARIANTS[tag]
    x, e, mask, g = M.module_inputs(tag, M.MODULE_SHAPE, int(gold[f"module_{tag}_seed"]))
    xb, gb = M.bf16_round(x), M.bf16_round(g)
    ref = M.forward_backward(xb, e, mask if with_mask else None, gb, cosine=cosine, activate_mask=activate)
    with rt.compute_dtype_ctx(torch.bfloat16):
        q = make(dev, e, use_cosine_sim=cosine, activate_mask_quantize=activate)
        r = run_module(dev, q, x, mask if with_mask else None, g)
    assert np.array_equal(r["idx"], ref["idx"])
    errs = {key: M.rel_to_max(r[key], ref[key]) for key in ("x_q", "dx", "dE")}
    errs["loss"] = abs(r["loss"] - ref["loss"]) / abs(ref["loss"])
    print(f"module {tag} bf16: relative-to-max errors {errs}")
    assert errs["loss"] < PARITY and errs["dE"] < PARITY, errs
    assert errs["x_q"] <= BF16_ULP and errs["dx"] <= BF16_ULP, errs


def test_module_surface(dev, gold):
    """get_codebook_entry (shape optional), embed_code_with_depth, the temperature reaching the search, strict loading of a
    reference-layout state dict"""
    x, e, mask, g = M.module_inputs("l2_mask", M.MODULE_SHAPE, int(gold["module_l2_mask_seed"]))
    b, d, h, w, k = M.MODULE_SHAPE
    q = make(dev, e)
    idx = T(gold["module_l2_mask_idx"], dev)
    ent = q.get_codebook_entry(idx)
    assert tuple(ent.shape) == (b, h, w, d) and np.array_equal(ent.cpu().numpy(), e[gold["module_l2_mask_idx"]])
    ent2 = q.get_codebook_entry(idx.reshape(-1), (b, h, w, d))
    assert tuple(ent2.shape) == (b, d, h, w) and torch.equal(ent2, ent.permute(0, 3, 1, 2))
    code = torch.stack([idx, (idx + 1) % k], dim=-1)
    emb, none = q.embed_code_with_depth(code)
    assert none is None and tuple(emb.shape) == (b, h, w, 2, d) and torch.equal(emb[..., 0, :], ent)
    # temperature: the explicit argument of forward() and the attribute fwd() falls back to
    with torch.no_grad():
        i0 = q(T(x, dev), 0.)[2][2]
        i1 = q(T(x, dev), 50.0)[2][2]
        q.sample_temperature = 50.0
        i2 = q.fwd(nhwc(x, dev, torch.float32), None, None)[2]
    assert np.array_equal(i0.cpu().numpy(), gold["module_l2_mask_idx"])
    assert float((i1 != i0).float().mean()) > 0.5 and float((i2 != i0).float().mean()) > 0.5
    sd = {"initted": torch.ones(1), "cluster_size": torch.zeros(1, k), "embedding.weight": torch.from_numpy(e) * 2}
    q.load_state_dict(sd, strict=True)
    assert np.array_equal(q.embedding.weight.detach().cpu().numpy(), e * 2)


# ---- 5. codebook gradient kernel ------------------------------------------------------------------------------------------------------
def _cbgrad_case(name):
    r = M.rng("cbgrad" + name)
    if name == "skewed":          # 90 % of the rows on one code, several slices, N no multiple of the slice
        n, k, d = 2 * 1024 + 700, 64, 256
        idx = np.where(r.uniform(size=n) < 0.9, 7, r.randint(0, k // 2, size=n))        # codes k/2 .. k-1 stay unused
    elif name == "d72":
        n, k, d = 1500, 40, 72
        idx = r.randint(0, 30, size=n)
    else:                         # fewer rows than one slice, every row its own weight
        n, k, d = 333, 16, 128
        idx = r.randint(0, k, size=n)
    x = r.standard_normal((n, d)).astype(np.float32)
    e = r.standard_normal((k, d)).astype(np.float32)
    m = r.uniform(0.1, 1.0, size=n).astype(np.float32)
    return x, e, idx.astype(np.int64), m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["skewed", "d72", "short"])
def test_codebook_grad_kernel(dev, name, dtype):
    from dynamicvectorquantization_amd import kernels as K
    x, e, idx, m = _cbgrad_case(name)
    n, d = x.shape
    k = e.shape[0]
    c = 0.37
    xt = T(x, dev).to(dtype)
    x64 = torch.from_numpy(x if dtype == torch.float32 else M.bf16_round(x)).double()
    e64, i64 = torch.from_numpy(e).double(), torch.from_numpy(idx)
    coef = torch.tensor([c], dtype=torch.float32, device=dev)
    # fp32 sums of up to n terms and one fused multiply-add each: n * 2^-23 relative to the largest entry is the worst case
    tol = n * 2.0 ** -23
    for mask in (m, None):
        mm = torch.from_numpy(mask).double() if mask is not None else torch.ones(n, dtype=torch.float64)
        ref = torch.zeros(k, d, dtype=torch.float64).index_add_(0, i64, c * mm[:, None] * (e64[i64] - x64))
        base = M.rng("cbgrad-base").standard_normal((k, d)).astype(np.float32)      # the kernel ACCUMULATES
        for det in (False, True):
            K.set_deterministic(det)
            try:
                outs = []
                for _ in range(2):
                    grad = T(base, dev)
                    K.vq_codebook_grad(xt, T(e, dev), T(idx, dev), None if mask is None else T(mask, dev), coef, grad)
                    outs.append(grad.cpu().numpy())
            finally:
                K.set_deterministic(False)
            got = outs[0].astype(np.float64) - base
            err = M.rel_to_max(got, ref.numpy())
            print(f"codebook grad {name} {dtype} mask={mask is not None} det={det}: rel-to-max error {err:.3g} (bound {tol:.3g})")
            assert err < tol
            unused = np.setdiff1d(np.arange(k), idx)
            assert len(unused) > 0 or name == "short"
            assert np.array_equal(outs[0][unused], base[unused])                  # unused codes: gradient exactly 0
            if det:
                assert np.array_equal(outs[0], outs[1])                           # bit-identical launches


# ---- 6. orthogonality term ------------------------------------------------------------------------------------------------------------
def test_orthogonality_term_golden(dev, gold):
    from dynamicvectorquantization_amd import _lib
    x, e, mask, g = M.module_inputs("ortho", M.ORTHO_SHAPE, int(gold["ortho_seed"]))
    calls = []
    old = _lib._launch_hook
    _lib._launch_hook = calls.append
    try:
        q = make(dev, e, orthogonal_reg_weight=M.ORTHO_W)
        r = run_module(dev, q, x, mask, g)
        with_term = list(calls)
        del calls[:]
        r0 = run_module(dev, make(dev, e, orthogonal_reg_weight=0.), x, mask, g)
        without = list(calls)
    finally:
        _lib._launch_hook = old
    assert sum(c.startswith("dvq_gemm") for c in with_term) == 2 and "dvq_vq_ortho_sumsq" in with_term
    assert not any(c.startswith("dvq_gemm") or "ortho" in c or "rownorm" in c for c in without), without
    assert np.array_equal(r["idx"], gold["ortho_idx"])
    e_loss = abs(r["loss"] - float(gold["ortho_loss"])) / abs(float(gold["ortho_loss"]))
    e_grad = M.rel_to_max(r["dE"], gold["ortho_dE"])
    # the term alone (difference of the two runs; the golden is the same difference of the reference's two runs)
    e_term = abs((r["loss"] - r0["loss"]) - float(gold["ortho_term"])) / abs(float(gold["ortho_term"]))
    e_tgrad = M.rel_to_max(r["dE"].astype(np.float64) - r0["dE"], gold["ortho_term_dE"])
    print(f"ortho: loss {e_loss:.3g}, grad {e_grad:.3g}, term alone {e_term:.3g}, its grad {e_tgrad:.3g}")
    assert max(e_loss, e_grad, e_term, e_tgrad) < PARITY


def test_orthogonality_term_bf16_mode(dev, gold):
    """bf16 compute: the regulariser's operands stay fp32 (its two GEMMs run on the fp32 codebook whatever the compute dtype), so the term
    alone -- the difference of a run with w = 10 and one with w = 0 -- still meets the golden at the parity bar"""
    from dynamicvectorquantization_amd import runtime as rt
    x, e, mask, g = M.module_inputs("ortho", M.ORTHO_SHAPE, int(gold["ortho_seed"]))
    with rt.compute_dtype_ctx(torch.bfloat16):
        r = run_module(dev, make(dev, e, orthogonal_reg_weight=M.ORTHO_W), x, mask, g)
        r0 = run_module(dev, make(dev, e, orthogonal_reg_weight=0.), x, mask, g)
    assert np.array_equal(r["idx"], r0["idx"])
    e_term = abs((r["loss"] - r0["loss"]) - float(gold["ortho_term"])) / abs(float(gold["ortho_term"]))
    e_tgrad = M.rel_to_max(r["dE"].astype(np.float64) - r0["dE"], gold["ortho_term_dE"])
    print(f"ortho, bf16 mode: term alone {e_term:.3g}, its grad {e_tgrad:.3g}")
    assert max(e_term, e_tgrad) < PARITY


# ---- 7. k-means initialisation ------------------------------------------------------------------------------------------------------------
def test_kmeans_init_golden(dev, gold):
    from dynamicvectorquantization_amd.config import get_obj_from_str
    b, d, h, w, k = M.KMEANS_SHAPE
    x, perm = M.kmeans_inputs(int(gold["kmeans_seed"]))
    q = get_obj_from_str(TARGET)(k, d, kmeans_init=True, kmeans_iters=M.KMEANS_ITERS).to(dev).train()
    assert not q.is_initted() and float(q.embedding.weight.abs().max()) == 0.0
    q.kmeans_perm = T(perm, dev)
    with torch.no_grad():
        _, _, (_, _, idx) = q(T(x, dev), 0.)
    err = M.rel_to_max(q.embedding.weight.detach().cpu().numpy(), gold["kmeans_weight"])
    print(f"kmeans: weight rel-to-max error {err:.3g}")
    assert err < 1e-5
    assert np.array_equal(q.cluster_size.cpu().numpy(), gold["kmeans_cluster_size"])
    assert float(q.initted) == 1.0 and q.is_initted()
    assert np.array_equal(idx.cpu().numpy(), gold["kmeans_idx"])
    w0 = q.embedding.weight.detach().clone()
    with torch.no_grad():
        q(T(x[:, :, ::-1].copy(), dev), 0.)                    # a second forward does not re-initialise
    assert torch.equal(q.embedding.weight.detach(), w0) and np.array_equal(q.cluster_size.cpu().numpy(), gold["kmeans_cluster_size"])


# ---- 8. model level -------------------------------------------------------------------------------------------------------------------
def build_model(dev, loss="dummy", trained=True, temperature=0.0):
    """the shrunken 64 x 64 DQ-VAE of dqvae_small.npz (test_gpu_model.GEOM['small']) with the deterministic parameters of that fixture;
    trained=True: carrying MaskVectorQuantize with the `spread` codebook"""
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from test_gpu_model import GEOM, model_config
    from test_oracle_golden import DQVAE_CFG, dqvae_state_dict
    cfg = copy.deepcopy(model_config(**GEOM["small"], loss=loss))
    k, zc = DQVAE_CFG["small"]["k"], DQVAE_CFG["small"]["zc"]
    if trained:
        cfg["params"]["vqconfig"] = {"target": TARGET, "params": dict(codebook_size=k, codebook_dim=zc, accept_image_fmap=True,
                                                                     commitment_beta=0.25, use_cosine_sim=False)}
    cfg["params"]["quant_sample_temperature"] = temperature
    model = instantiate_from_config(cfg).to(dev)
    sd = dqvae_state_dict(load_golden("dqvae_small"), "spread", k, zc)
    if trained:
        cbw = sd.pop("quantize.codebook.weight")
        sd = {kk: v for kk, v in sd.items() if not kk.startswith("quantize.")}
        sd["quantize.embedding.weight"] = cbw[:k].clone()
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    assert all(m.startswith("loss.") or m in ("quantize.initted", "quantize.cluster_size") for m in res.missing_keys), res.missing_keys
    return model


def test_model_forward_backward_golden(dev, gold):
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.quantize_trained import MaskVectorQuantize
    x = T(synth.half_flat_images(2, 64, seed=4321), dev)
    with rt.compute_dtype_ctx(torch.float32):
        model = build_model(dev).eval()
        assert isinstance(model.quantize, MaskVectorQuantize)
        rec, qloss, grain, gate, ent = model(x)
        assert np.array_equal(grain.cpu().numpy(), gold["model_grain"])
        assert np.array_equal(model._last["codes"].cpu().numpy(), gold["model_codes"])
        gout = T(synth.det_param("dqvae.small.gout", tuple(rec.shape)), dev)
        ((rec * gout).sum() / rec.numel() * 100.0 + qloss).backward()
        params = dict(model.named_parameters())
        errs = {"rec": M.rel_to_max(rec.detach().cpu().numpy(), gold["model_rec"]),
                "qloss": abs(float(qloss) - float(gold["model_qloss"])) / abs(float(gold["model_qloss"])),
                "embedding.grad": M.rel_to_max(params["quantize.embedding.weight"].grad.cpu().numpy(), gold["model_grad_embedding"]),
                "encoder.conv_in.grad": M.rel_to_max(params["encoder.conv_in.weight"].grad.cpu().numpy(), gold["model_grad_encoder_conv_in"]),
                "decoder.conv_out.grad": M.rel_to_max(params["decoder.conv_out.weight"].grad.cpu().numpy(),
                                                      gold["model_grad_decoder_conv_out"])}
        print(f"model level: relative-to-max errors {errs}")
        assert all(v < PARITY for v in errs.values()), errs
        emb = model.get_code_emb_with_depth(model._last["codes"])
        assert tuple(emb.shape) == (2, 8, 8, 64)


def test_model_sampling_temperature_reaches_the_search(dev, gold):
    """quant_sample_temperature > 0: ae_fwd samples (most codes leave the argmax, two forwards differ: the counter advanced); the model's
    attribute is the one source -- set back to 0 after construction, the golden's codes return"""
    from dynamicvectorquantization_amd import runtime as rt
    x = T(synth.half_flat_images(2, 64, seed=4321), dev)
    with rt.compute_dtype_ctx(torch.float32), torch.no_grad():
        model = build_model(dev, temperature=200.0).eval()
        c1 = model.ae_fwd(x, None)["codes"].cpu().numpy()
        c2 = model.ae_fwd(x, None)["codes"].cpu().numpy()
        moved = float((c1 != gold["model_codes"]).mean())
        print(f"model at temperature 200: {moved:.3f} of the codes left the argmax, {float((c1 != c2).mean()):.3f} differ between two forwards")
        assert moved > 0.5 and float((c1 != c2).mean()) > 0.5
        model.quant_sample_temperature = 0.0
        assert np.array_equal(model.ae_fwd(x, None)["codes"].cpu().numpy(), gold["model_codes"])


def _train(dev, use_graph, steps=3):
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.trainer import Trainer
    xs = [T(synth.half_flat_images(2, 64, seed=40 + i), dev) for i in range(3)]
    with rt.compute_dtype_ctx(torch.float32):
        torch.manual_seed(0)
        model = build_model(dev, loss="ae")
        model.learning_rate, model.min_learning_rate = 2e-4, 1e-5
        model.training_steps, model.steps_per_epoch, model.warmup_epochs = 12, 4, 1
        model.train()
        w0 = model.quantize.embedding.weight.detach().clone()
        tr = Trainer(model, max_steps=12, use_graph=use_graph, graph_after=2)      # as tests/test_gpu_stepgraph.py: two eager steps, then the recording
        losses = [[float(l) for l in tr.train_step({"image": xs[i % 3]}, i)] for i in range(steps)]
        torch.cuda.synchronize()
    return model, tr, np.array(losses), w0


def test_model_trainer_steps_eager_vs_recorded(dev):
    """three Trainer steps of the autoencoder objective: the recorded step does what the eager one does (the tolerances
    tests/test_gpu_stepgraph.py applies to the EMA model's `ae` case), the codebook is trained by the optimizer"""
    steps = 3
    m_e, tr_e, l_e, w0 = _train(dev, False, steps)
    m_g, tr_g, l_g, _ = _train(dev, True, steps)
    assert tr_e.graph_replays == 0 and tr_g._graph is not None and tr_g.graph_replays == steps - 2, tr_g.graph_replays
    tl, tp, lr_max = 2e-3, 2e-3, 2e-4
    np.testing.assert_allclose(l_g, l_e, rtol=tl, atol=tl / 10)
    for (n1, p1), (_, p2) in zip(m_g.named_parameters(), m_e.named_parameters()):
        a, b = p1.detach().float(), p2.detach().float()
        assert float((a - b).norm()) <= tp * float(b.norm()) + 0.05 * lr_max * steps * a.numel() ** 0.5, n1
    for og, oe in zip(tr_g.opts, tr_e.opts):
        assert float((og._fstate["m"] - oe._fstate["m"]).norm()) <= 10 * tp * float(oe._fstate["m"].norm()) + 1e-9
    for m, tr in ((m_e, tr_e), (m_g, tr_g)):
        w, opt = m.quantize.embedding.weight, tr.opts[0]
        assert float((w.detach() - w0).abs().max()) > 0.0                       # the embedding weight has moved
        assert any(p is w for grp in opt.param_groups for p in grp["params"])
        # the optimizer state holds the embedding: its slice of the flat Adam moments is non-zero on the used code rows
        off = 0
        for p in opt.flat.params:
            if p is w:
                break
            off += p.numel()
        else:
            raise AssertionError("the embedding is not in the optimizer's flat parameter buffer")
        m1 = opt._fstate["m"][off:off + w.numel()].view(w.shape)
        used = m1.abs().amax(dim=1) > 0
        assert 0 < int(used.sum()) < w.shape[0]                                 # used rows have moments, unused rows none


# ---- 9. surroundings -----------------------------------------------------------------------------------------------------------------------
def test_surroundings_work_with_either_quantiser(dev):
    from dynamicvectorquantization_amd import evaluate as E
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd import tokens as TK
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    x = T(synth.half_flat_images(2, 64, seed=4321), dev)
    with rt.compute_dtype_ctx(torch.float32):
        for trained in (True, False):
            model = build_model(dev, trained=trained).eval()
            model.hw1, model.hw2 = 4, 8
            s = E.evaluate_reconstruction(model, [x], lpips=False)
            with torch.no_grad():
                out = model.ae_fwd(x, None)
            codes, grain = out["codes"].cpu().numpy(), out["grain"].cpu().numpy()
            used = len(np.unique(codes))      # a coarse cell repeats its one code over its 2 x 2 block of the code map
            assert s["codes_used"] == used and s["n_images"] == 2 and abs(s["used_fraction"] - used / 512) < 1e-12
            desc, fp = TK.describe_model(model), TK.first_stage_fingerprint(model)
            emb = model.get_code_emb_with_depth(out["codes"])
            assert tuple(emb.shape) == (2, 8, 8, 64)
            thr = model.encoder.router.fine_grain_threshold
            if trained:
                w = model.quantize.embedding.weight
                assert s["ema_dead_codes"] is None
                assert desc["codebook_size"] == 512
            else:       # what these calls gave before: the values computed through quantize.codebook directly
                assert isinstance(model.quantize, VectorQuantize2)
                w = model.quantize.codebook.weight
                assert desc["codebook_size"] == model.quantize.codebook.n_embed
                assert s["ema_dead_codes"] == int((model.quantize.codebook.cluster_size_ema.cpu().numpy() < 1.0).sum())
            assert fp == desc["fingerprint"] == TK.fingerprint_arrays(w.detach().float().cpu().numpy(), thr)
            assert np.array_equal(emb.cpu().numpy(), w.detach().cpu().numpy()[codes])
