"""Deterministic mode (kernels.set_deterministic / Trainer(deterministic=True), docs/design/21-reproducible-training.md) on the GPU.

Per reduction family, at the smallest shape with several writers per address:
  (a) mode off: kernels.unordered_launches() moves -- the shape really takes a path whose result depends on arrival order;
  (b) mode on: the count stays put and five identical launches give torch.equal outputs;
  (c) the ordered result meets, against an fp64 reference, the bound the family's existing test applies to the default path
      (test_gpu_kernels.py / test_gpu_stage2.py / test_gpu_fullsize.py; named at each case).
Then: the mode without a registered workspace, whole training steps of stage 1 and stage 2 run twice, and the mode switched off again."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, load_golden
from dynamicvectorquantization_amd import synth

pytestmark = pytest.mark.gpu


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def _family(launch, check=None, expect_unordered=True):
    """launch() -> list of result tensors (fresh accumulators every call).  Runs (a), (b), (c) and returns the ordered result."""
    from dynamicvectorquantization_amd import kernels as K
    try:
        K.set_deterministic(False)
        c0 = K.unordered_launches()
        off = [t.clone() for t in launch()]
        torch.cuda.synchronize()
        if expect_unordered:
            assert K.unordered_launches() > c0, "mode off: no unordered launch was counted -- this shape has one writer per address"
        K.set_deterministic(True)
        c1 = K.unordered_launches()
        runs = [[t.clone() for t in launch()] for _ in range(5)]
        torch.cuda.synchronize()
        assert K.unordered_launches() == c1, "deterministic mode took an unordered path"
    finally:
        K.set_deterministic(False)
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b), "deterministic mode: identical launches differ"
    if check is not None:
        check(runs[0])
        check(off)
    return runs[0]


def _relfro(got, ref):
    got, ref = got.double().cpu().numpy(), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref)) / max(1e-30, float(np.linalg.norm(ref)))


# ---- GroupNorm / BatchNorm statistics and backward sums ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", [64, 96], ids=["64x64-64rows", "96x96-1024rows"])
def test_groupnorm_ordered(dev, dtype, hw):
    """N 2, C 64, G 32: 64 x 64 (64-row blocks, 64 per image) and 96 x 96 (1024-row blocks, 9 per image).  Bounds of test_groupnorm."""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.layers import Normalize
    n, c = 2, 64
    rs = np.random.RandomState(c + hw)
    shape = (n, c, hw, hw)
    x = (rs.standard_normal(shape) * 2 + 0.5).astype(np.float32)
    gam = (1 + 0.2 * rs.standard_normal(c)).astype(np.float32)
    bet = (0.2 * rs.standard_normal(c)).astype(np.float32)
    go = rs.standard_normal(shape).astype(np.float32)
    if dtype == torch.bfloat16:
        x, go = bf16_round(x), bf16_round(go)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    gr, br = torch.from_numpy(gam).double().requires_grad_(True), torch.from_numpy(bet).double().requires_grad_(True)
    yr = F.group_norm(xr, 32, gr, br, 1e-6)
    yr = yr * torch.sigmoid(yr)
    (yr * torch.from_numpy(go).double()).sum().backward()
    mod = Normalize(c).to(dev)
    mod.fuse_silu = True
    with torch.no_grad():
        mod.weight.copy_(T(gam, dev))
        mod.bias.copy_(T(bet, dev))
    xd, god = T(x, dev), T(go, dev)

    def launch():
        mod.weight.grad = mod.bias.grad = None
        with rt.compute_dtype_ctx(dtype):
            xt = xd.clone().requires_grad_(True)
            y = mod(xt)
            (y.float() * god).sum().backward()
        return [y.detach().float(), xt.grad.float(), mod.weight.grad.clone(), mod.bias.grad.clone()]

    def check(out):
        y, dx, dg, db = out
        tol = dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)
        np.testing.assert_allclose(y.cpu().numpy(), yr.detach().numpy(), **tol)
        np.testing.assert_allclose(dx.cpu().numpy(), xr.grad.numpy(), **tol)
        scale = max(1.0, float(np.abs(gr.grad.numpy()).max()))
        gtol = 2e-4 if dtype == torch.float32 else 3e-2
        np.testing.assert_allclose(dg.cpu().numpy() / scale, gr.grad.numpy() / scale, atol=gtol)
        np.testing.assert_allclose(db.cpu().numpy() / scale, br.grad.numpy() / scale, atol=gtol)

    _family(launch, check)


def test_gn_stats_kernel_ordered(dev):
    """dvq_gn_stats alone, channels per group 2 / 8 / 12 (a thread's 8 channels in 4 / 1 / 2 groups).  A thread adds the m = pixels per
    block / pixel rows per pass values of a channel in fp32 before anything is combined in fp64: first-order worst case m 2^-24 sum|x|"""
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(5)
    for c, g, hw in ((64, 32, 64 * 64), (256, 32, 70 * 70), (96, 8, 33 * 31)):
        x = T(rs.standard_normal((2, hw, c)).astype(np.float32), dev)
        v = x.double().view(2, hw, g, c // g)
        ref = torch.stack([v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], -1).cpu().numpy()
        m = -(-(1024 if hw > 4096 else 64) // (256 // (c // 8)))
        bound = m * 2.0 ** -24 * torch.stack([v.abs().sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], -1).cpu().numpy()

        def check(out):
            assert (np.abs(out[0].cpu().numpy().reshape(2, g, 2) - ref) <= bound).all()

        _family(lambda: [K.gn_stats(x, g)], check)


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------
def test_layernorm_backward_ordered(dev):
    """600 rows x 256: 150 workgroups, three 64-row blocks of the fold.  Bound: the parameter-gradient bound of test_stackgpt_golden
    (fp32: relative Frobenius error 5e-3)"""
    from dynamicvectorquantization_amd import kernels as K
    rows, c = 600, 256
    rs = np.random.RandomState(7)
    x = rs.standard_normal((rows, c)).astype(np.float32)
    dy = rs.standard_normal((rows, c)).astype(np.float32)
    gamma = (rs.rand(c) + 0.5).astype(np.float32)
    xd = x.astype(np.float64)
    mean, var = xd.mean(1, keepdims=True), xd.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    xh = (xd - mean) * rstd
    dg_ref, db_ref = (dy * xh).sum(0), dy.astype(np.float64).sum(0)
    gg = dy * gamma.astype(np.float64)
    dx_ref = rstd * (gg - gg.mean(1, keepdims=True) - xh * (gg * xh).mean(1, keepdims=True))
    xt, dyt, gt = T(x, dev), T(dy, dev), T(gamma, dev)
    mr = T(np.concatenate([mean, rstd], 1).astype(np.float32), dev)

    def launch():
        dg, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
        dx = K.layernorm_bwd(xt, dyt, mr, gt, dg, db)
        return [dx, dg, db]

    def check(out):
        for got, ref in zip(out, (dx_ref, dg_ref, db_ref)):
            assert _relfro(got, ref) < 5e-3

    _family(launch, check)


# ---- embedding gradient -----------------------------------------------------------------------------------------------------------
def test_embedding_gradient_ordered(dev):
    """800 indices drawn from 16 rows, C 64 (row 3 is the padding row).  Bound: test_stackgpt_golden's 5e-3"""
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(11)
    b, ln, c, v = 8, 100, 64, 16
    idx = rs.randint(0, v, (b, ln)).astype(np.int64)
    dout = rs.standard_normal((b, ln, c)).astype(np.float32)
    ref = np.zeros((v, c))
    np.add.at(ref, idx.reshape(-1), dout.reshape(-1, c).astype(np.float64))
    ref[3] = 0.0
    it, dt_ = T(idx, dev), T(dout, dev)

    def launch():
        dtable = torch.zeros(v, c, device=dev)
        K.embed_scatter_add(it, dt_, dtable, 0, padding_idx=3)
        return [dtable]

    def check(out):
        assert _relfro(out[0], ref) < 5e-3 and float(out[0][3].abs().max()) == 0.0

    _family(launch, check)


# ---- cross entropy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldl", [1027, 1032], ids=["scalar-rows", "vector-rows"])
def test_cross_entropy_ordered(dev, ldl):
    """1000 rows x 1027 classes (250 workgroups), every seventh row ignored.  Bound: the loss bound of test_stackgpt_golden (fp32 2e-4);
    the returned dlogits per element with the cross-entropy bound of test_gpu_stage2_kernels.py (docs/design/25-stage2-kernel-pins.md),
    exact zeros in its ignored rows and in the padding columns of the ldl = 1032 case"""
    from dynamicvectorquantization_amd import kernels as K
    from test_gpu_stage2_kernels import ce_grad_check
    rs = np.random.RandomState(13)
    rows, v = 1000, 1027
    logits = np.zeros((rows, ldl), dtype=np.float32)
    logits[:, :v] = rs.standard_normal((rows, v)).astype(np.float32) * 3
    target = rs.randint(0, v, rows).astype(np.int64)
    target[::7] = -100
    lp = torch.log_softmax(torch.from_numpy(logits[:, :v]).double(), 1).numpy()
    keep = target != -100
    ref_sum, ref_cnt = float(-lp[np.arange(rows)[keep], target[keep]].sum()), float(keep.sum())
    lt, tt = T(logits, dev), T(target, dev)
    gs = torch.ones(1, device=dev)

    def launch():
        ls, cnt = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        dl = K.cross_entropy(lt, v, tt, -100, ls, cnt, gscale=gs, want_grad=True)
        return [ls, cnt, dl]

    def check(out):
        np.testing.assert_allclose(float(out[0]), ref_sum, rtol=2e-4)
        assert float(out[1]) == ref_cnt
        ce_grad_check(logits, v, target, 1.0, out[2], torch.float32, f"ordered ldl {ldl}", ignore_index=-100)

    _family(launch, check)


# ---- column / batch sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5000, 96), (3000, 12)], ids=["5000x96-vector", "3000x12-scalar"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sum_batch_ordered(dev, shape, dtype):
    """bound of test_sum_batch"""
    from dynamicvectorquantization_amd import kernels as K
    rows, inner = shape
    rs = np.random.RandomState(rows + inner)
    x = rs.standard_normal((rows, inner)).astype(np.float32)
    if dtype == torch.bfloat16:
        x = bf16_round(x)
    init = rs.standard_normal(inner).astype(np.float32)
    ref = init.astype(np.float64) + x.astype(np.float64).sum(axis=0)
    xt = T(x, dev, dtype)

    def check(out):
        np.testing.assert_allclose(out[0].cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.sqrt(rows))

    _family(lambda: [K.sum_batch(xt, T(init, dev))], check)


# ---- weight gradients: fp32 operands, batched TN -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
def test_fp32_weight_gradient_ordered(dev, mode):
    """3 x 3, 64 -> 64 channels on 2 x 32 x 32 with fp32 operands (the parity mode's register-staged TN kernel: 16 splits, and the
    column sums of the bias gradient from eight row blocks of one workgroup).  Bound of test_conv (fp32: 5e-4 of the largest element)"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.layers import Conv2d
    cin, cout, h, n = 64, 64, 32, 2
    rs = np.random.RandomState(17)
    x = rs.standard_normal((n, cin, h, h)).astype(np.float32)
    go = rs.standard_normal((n, cout, h, h)).astype(np.float32)
    xr = torch.from_numpy(x).double()
    wr = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xr, wr, br, padding=1) * torch.from_numpy(go).double()).sum().backward()
    mod = Conv2d(cin, cout, 3, 1, 1).to(dev)
    xd, god = T(x, dev), T(go, dev)

    def launch():
        mod.weight.grad = mod.bias.grad = None
        with rt.compute_dtype_ctx(mode):
            y = mod(xd.clone().requires_grad_(True))
            (y.float() * god).sum().backward()
            rt.join_side()
        return [mod.weight.grad.clone(), mod.bias.grad.clone()]

    def check(out):
        gtol = 5e-4 if mode == "fp32" else 5e-3          # (fp32x3: products at ~2^-17, test_fp32_split_bf16_products)
        for got, ref in zip(out, (wr.grad.numpy(), br.grad.numpy())):
            assert float(np.abs(got.cpu().numpy() - ref).max()) / float(np.abs(ref).max()) < gtol

    # fp32x3 runs the bf16 weight-gradient kernels on split planes: their default path may fold through the workspace already
    _family(launch, check, expect_unordered=mode == "fp32")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batched_tn_ordered(dev, dtype):
    """three 520 x 72 x 40 TN products in one launch: the launcher splits the reduction five ways.  Bound of test_gemm_nt_tn"""
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(3)
    b, mred, i, j = 3, 520, 72, 40
    a2 = rs.standard_normal((b, mred, i)).astype(np.float32)
    b2 = rs.standard_normal((b, mred, j)).astype(np.float32)
    if dtype == torch.bfloat16:
        a2, b2 = bf16_round(a2), bf16_round(b2)
    ref2 = np.einsum("bmi,bmj->bij", a2.astype(np.float64), b2.astype(np.float64))
    at, bt = T(a2, dev, dtype), T(b2, dev, dtype)

    def check(out):
        err = np.abs(out[0].cpu().numpy().reshape(b, i, j) - ref2).max() / np.abs(ref2).max()
        assert err < (1e-4 if dtype == torch.float32 else 3e-2), err

    _family(lambda: [K.gemm_tn(at, bt, mred, i, j, i, j, j, batch=b, sa=mred * i, sb=mred * j, sc=i * j)], check)


# ---- VQ: EMA statistics under skewed code usage, commitment-loss sum -----------------------------------------------------------------
def test_vq_ema_statistics_ordered(dev):
    """4096 rows in four slices, 64 codes, 70 % of the rows on code 3.  Bound of test_vq_ema_golden (sums rtol 1e-4 / atol 1e-5, counts exact)"""
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(19)
    n, k, d = 4096, 64, 64
    idx = rs.randint(0, k, n).astype(np.int64)
    idx[rs.rand(n) < 0.7] = 3
    x = rs.standard_normal((n, d)).astype(np.float32)
    ref = np.zeros((k, d + 1))
    np.add.at(ref[:, :d], idx, x.astype(np.float64))
    np.add.at(ref[:, d], idx, 1.0)
    xt, it = T(x, dev), T(idx, dev)

    def check(out):
        got = out[0].cpu().numpy()
        np.testing.assert_allclose(got[:, :d], ref[:, :d], rtol=1e-4, atol=1e-5 * np.sqrt(n))
        assert np.array_equal(got[:, d], ref[:, d])

    _family(lambda: [K.vq_ema_stats(xt, it, k)], check)


def test_scalar_loss_sums_ordered(dev):
    """the commitment-loss sum (bound of test_vq_forward_golden: rtol 1e-5), the L1 sum and one LPIPS head (fp64 / fp32 partials per
    workgroup; no existing bound of their own: (a) and (b) only)"""
    from dynamicvectorquantization_amd import kernels as K
    rs = np.random.RandomState(23)
    n, d, k = 2048, 64, 32
    x, cb = rs.standard_normal((n, d)).astype(np.float32), rs.standard_normal((k, d)).astype(np.float32)
    idx = rs.randint(0, k, n).astype(np.int64)
    ref = float(((cb[idx].astype(np.float64) - x) ** 2).sum())
    xt, ct, it = T(x, dev), T(cb, dev), T(idx, dev)
    xq_ref = x + (cb[idx] - x)                 # fp32 throughout: the straight-through value the kernel stores

    def check(out):
        np.testing.assert_allclose(float(out[0]), ref, rtol=1e-5)
        assert np.array_equal(out[1].cpu().numpy().view(np.uint32), xq_ref.view(np.uint32)), "x_q is not fl(x + fl(e - x)) bit for bit"

    _family(lambda: list(K.vq_gather_loss(xt, ct, it)[::-1]), check)
    a, b = T(rs.standard_normal(2 * 3 * 64 * 64).astype(np.float32), dev), T(rs.standard_normal(2 * 3 * 64 * 64).astype(np.float32), dev)
    _family(lambda: [K.l1_loss(a, b)[0]])
    f0 = T(np.abs(rs.standard_normal((2, 32, 32, 64))).astype(np.float32), dev)
    f1 = T(np.abs(rs.standard_normal((2, 32, 32, 64))).astype(np.float32), dev)
    lin = T(rs.rand(64).astype(np.float32), dev)

    def head():
        val = torch.zeros(2, device=dev)
        K.lpips_head(f0, f1, lin, val)
        return [val]
    _family(head)


# ---- the halo convolution with its statistics epilogue --------------------------------------------------------------------------------
def _no_workspace(monkeypatch):
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd._lib import check
    check(K.lib().dvq_set_workspace(None, 0), "dvq_set_workspace")
    K._workspace.clear()
    monkeypatch.setattr(K, "ensure_workspace", lambda device: None)


def test_halo_statistics_epilogue_ordered(dev, monkeypatch):
    """2 x 32 x 32 x 64 -> 64 with GroupNorm statistics of the output.  With a registered workspace the epilogue stores per-tile
    partials and a wave folds them in tile order -- ordered in both modes.  Without one every tile adds with fp64 atomics: counted
    with the mode off, refused (DVQ_EWORKSPACE) with the mode on.  Bound of test_conv3x3_values_full_size (2e-4 of |sum| + 1)"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd._lib import DvqError
    from dynamicvectorquantization_amd.layers import Conv2d
    torch.manual_seed(1)
    with rt.compute_dtype_ctx(torch.bfloat16):
        conv = Conv2d(64, 64, 3, 1, 1).to(dev)
        w, wt, bias = conv.packed(torch.bfloat16)
        x = torch.randn(2, 32, 32, 64, device=dev).to(torch.bfloat16)
        d = conv._desc(x)

        def launch():
            st = torch.zeros(2, 32, 2, dtype=torch.float64, device=dev)
            return [K.conv2d_fwd(d, x, w, bias, None, out_stats=st, out_groups=32), st]

        def check(out):
            y, st = out
            v = y.double().view(2, 32 * 32, 32, 2)
            ref = torch.stack([v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], -1)
            assert float(((st - ref).abs() / (ref.abs() + 1.0)).max()) < 2e-4

        K.ensure_workspace(dev)
        _family(launch, check, expect_unordered=False)
        _no_workspace(monkeypatch)
        try:
            c0 = K.unordered_launches()
            check(launch())
            assert K.unordered_launches() > c0
            K.set_deterministic(True)
            c1 = K.unordered_launches()
            with pytest.raises(DvqError):
                launch()
            assert K.unordered_launches() == c1
        finally:
            K.set_deterministic(False)


# ---- deterministic mode without a registered workspace -------------------------------------------------------------------------------
def test_deterministic_without_workspace_takes_no_unordered_path(dev, monkeypatch):
    """no scratch for partials: every family launches unsplit (one owner per output element) -- the count stays put, launches repeat
    bit for bit, and the values stay within the default path's bounds"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.layers import Conv2d, Normalize
    _no_workspace(monkeypatch)
    rs = np.random.RandomState(29)
    xs = T(rs.standard_normal((5000, 96)).astype(np.float32), dev)
    logits = T(rs.standard_normal((1000, 1032)).astype(np.float32), dev)
    target = T(rs.randint(0, 1027, 1000).astype(np.int64), dev)
    a2, b2 = T(rs.standard_normal((3, 520, 72)).astype(np.float32), dev), T(rs.standard_normal((3, 520, 40)).astype(np.float32), dev)
    xl, dyl = T(rs.standard_normal((600, 256)).astype(np.float32), dev), T(rs.standard_normal((600, 256)).astype(np.float32), dev)
    mr = torch.stack([xl.mean(1), 1.0 / (xl.var(1, unbiased=False) + 1e-5).sqrt()], 1).contiguous()
    gl = torch.ones(256, device=dev)
    norm = Normalize(64).to(dev)
    conv = Conv2d(64, 64, 3, 1, 1).to(dev)
    xg = T(rs.standard_normal((2, 64, 64, 64)).astype(np.float32), dev)
    xi = T(rs.standard_normal(2 * 3 * 64 * 64).astype(np.float32), dev)
    go = T(rs.standard_normal((2, 64, 64, 64)).astype(np.float32), dev)

    def launch():
        out = [K.sum_batch(xs, torch.zeros(96, device=dev))]
        ls, cnt = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        K.cross_entropy(logits, 1027, target, -100, ls, cnt)
        out += [ls, cnt, K.gemm_tn(a2, b2, 520, 72, 40, 72, 40, 40, batch=3, sa=520 * 72, sb=520 * 40, sc=72 * 40)]
        dg, db = torch.zeros(256, device=dev), torch.zeros(256, device=dev)
        out += [K.layernorm_bwd(xl, dyl, mr, gl, dg, db), dg, db, K.gn_stats(xg.permute(0, 2, 3, 1).contiguous(), 32), K.l1_loss(xi, xi * 0.5)[0]]
        for mode, mod in (("fp32", norm), ("fp32", conv), ("bf16", conv)):
            mod.weight.grad = mod.bias.grad = None
            with rt.compute_dtype_ctx(mode):
                xt = xg.clone().requires_grad_(True)
                (mod(xt).float() * go).sum().backward()
                rt.join_side()
            out += [xt.grad.float(), mod.weight.grad.clone(), mod.bias.grad.clone()]
        return out

    try:
        K.set_deterministic(False)
        ref = [t.clone() for t in launch()]
        K.set_deterministic(True)
        c0 = K.unordered_launches()
        runs = [[t.clone() for t in launch()] for _ in range(3)]
        torch.cuda.synchronize()
        assert K.unordered_launches() == c0
    finally:
        K.set_deterministic(False)
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)
    for i, (a, b) in enumerate(zip(runs[0], ref)):            # same sums in another order: rounding apart (bf16 conv: its operands' 2^-8)
        assert float((a.double() - b.double()).norm()) <= 2e-2 * float(b.double().norm()) + 1e-6, i


# ---- whole training steps ------------------------------------------------------------------------------------------------------------
def _two_runs(fn):
    """fn() twice in deterministic mode -> the two records and the counter's movement across the second run"""
    from dynamicvectorquantization_amd import kernels as K
    try:
        K.set_deterministic(True)
        a = fn()
        torch.cuda.synchronize()
        c0 = K.unordered_launches()
        b = fn()
        torch.cuda.synchronize()
        moved = K.unordered_launches() - c0
    finally:
        K.set_deterministic(False)
    return a, b, moved


def _assert_records_equal(a, b):
    assert sorted(a) == sorted(b)
    diff = [k for k in sorted(a) if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]
    assert not diff, f"{len(diff)} of {len(a)} keys differ between two runs, first: {diff[:8]}"


@pytest.mark.parametrize("tag,mode", [("small", "bf16"), ("small", "fp32"), ("small", "fp32x3"), ("triple", "bf16")],
                         ids=["small-bf16", "small-fp32", "small-fp32x3", "triple-bf16"])
def test_train_steps_bit_reproducible(dev, tag, mode):
    """the pinned stage-1 run of tests/test_gpu_trainstep.py twice: every key of the two records -- losses, logged scalars, codes, EMA
    state, sampled gradients, parameters, both Adam moments -- is bit-equal, and no unordered launch is counted"""
    from dynamicvectorquantization_amd import runtime as rt
    from test_gpu_trainstep import run_hip_train_steps

    def run():
        rt.reseed_draws()
        return run_hip_train_steps(tag, dev, mode)

    a, b, moved = _two_runs(run)
    assert moved == 0, f"{moved} unordered launches in a deterministic run"
    _assert_records_equal(a, b)


def _small_recorded_run(dev, mode, steps=6):
    """the `small` model of the pinned run under Trainer(use_graph=True, deterministic=True): two eager steps, the recording, replays
    (run_hip_train_steps reads tensors back from inside optimizer.step, which a recording cannot hold)"""
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.trainer import Trainer
    from golden_cfg import TRAIN_STEP, TRAIN_STEP_WATCH
    from test_gpu_model import GEOM, model_config
    c = TRAIN_STEP["small"]
    g = GEOM[c["geom"]]
    out = {}
    with rt.compute_dtype_ctx(mode):
        torch.manual_seed(0)
        model = instantiate_from_config(model_config(**g, loss="full", ndf=c["ndf"])).to(dev)
        synth.apply_train_step_state(model, g["k"], g["zc"])
        rt.bump_weights_epoch()
        model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
        model.warmup_epochs, model.steps_per_epoch, model.training_steps = c["warmup_epochs"], c["steps_per_epoch"], c["training_steps"]
        model.train()
        tr = Trainer(model, max_steps=steps, use_graph=True, graph_after=2, deterministic=True)
        params = dict(model.named_parameters())
        cbm = model.quantize.codebook
        for step, xb in enumerate(synth.train_step_batches(steps, c["bs"], g["resolution"])):
            losses = tr.train_step({"image": torch.from_numpy(xb).to(dev)}, step)
            torch.cuda.synchronize()
            for oi, l in enumerate(losses):
                out[f"s{step}.o{oi}.loss"] = np.float32(float(l))
            for k_, v_ in model._logged.items():
                out[f"s{step}.log.{k_}"] = np.float32(float(v_))
            out[f"s{step}.codes"] = model._last["codes"].reshape(-1).cpu().numpy().copy()
            for n_, b_ in (("cluster_size_ema", cbm.cluster_size_ema), ("embed_ema", cbm.embed_ema), ("codebook", cbm.weight)):
                out[f"s{step}.{n_}"] = b_.detach().cpu().numpy().copy()
            for n_ in TRAIN_STEP_WATCH:
                out[f"s{step}.param.{n_}"] = params[n_].detach().cpu().numpy().copy()
                out[f"s{step}.grad.{n_}"] = params[n_].grad.detach().cpu().numpy().copy()
            for oi, o in enumerate(tr.opts):
                out[f"s{step}.o{oi}.exp_avg"] = o._fstate["m"].cpu().numpy().copy()
                out[f"s{step}.o{oi}.exp_avg_sq"] = o._fstate["v"].cpu().numpy().copy()
        assert tr.use_graph and tr.graph_replays >= 3, (tr.use_graph, tr.graph_replays)
    return out


def test_recorded_train_steps_bit_reproducible(dev):
    """(`small`, fp32) with the step recorded and replayed: both runs replay their own recording, every tensor stays bit-equal"""
    a, b, moved = _two_runs(lambda: _small_recorded_run(dev, "fp32"))
    assert moved == 0, f"{moved} unordered launches in a deterministic run"
    _assert_records_equal(a, b)


def _dualformer_run(dev, mode, pdrop):
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.config import instantiate_from_config
    from dynamicvectorquantization_amd.trainer import Trainer
    from golden_cfg import TRAIN_STEP_S2, TRAIN_STEP_S2_WATCH, dualformer_cfg, train_step_s2_batch
    from test_oracle_golden import dqvae_state_dict
    c = TRAIN_STEP_S2
    thr_json = os.path.join(REPO, "scripts/tools/thresholds/entropy_thresholds_imagenet_train_patch-16.json")
    out = {}
    with rt.compute_dtype_ctx(mode):
        torch.manual_seed(0)
        cfg = dualformer_cfg("uncond", thr_json)
        cfg["weight_decay"], cfg["warmup_epochs"] = c["weight_decay"], c["warmup_epochs"]
        if pdrop is not None:
            for k_ in ("embd_pdrop", "resid_pdrop", "attn_pdrop"):
                cfg["transformer_config"]["params"][k_] = pdrop
        model = instantiate_from_config({"target": "models.stage2_dynamic.dqtransformer_uncond_entropy.Dualformer", "params": cfg}).to(dev)
        model.first_stage_model.load_state_dict(dqvae_state_dict(load_golden("dqvae_small"), "spread", 512, 64))
        with torch.no_grad():
            for n, p in model.transformer.named_parameters():
                v = synth.det_param("dualformer.uncond." + n, tuple(p.shape))
                p.copy_(torch.from_numpy(v * (0.3 if n == "pos_emb" else 1.0)).to(dev))
        rt.bump_weights_epoch()
        model.learning_rate, model.min_learning_rate = c["lr"], c["min_lr"]
        model.steps_per_epoch, model.training_steps = c["steps_per_epoch"], c["training_steps"]
        model.train()
        tr = Trainer(model, max_steps=c["steps"], use_graph=False, deterministic=True)
        (opt,) = tr.opts
        params = dict(model.transformer.named_parameters())
        for step in range(c["steps"]):
            (loss,) = tr.train_step({"image": torch.from_numpy(train_step_s2_batch(step)).to(dev)}, step)
            torch.cuda.synchronize()
            out[f"s{step}.loss"] = np.float32(float(loss))
            for k_, v_ in model._logged.items():
                out[f"s{step}.log.{k_}"] = np.float32(float(v_))
            for n_ in TRAIN_STEP_S2_WATCH:
                out[f"s{step}.grad.{n_}"] = params[n_].grad.detach().cpu().numpy().copy()
                out[f"s{step}.param.{n_}"] = params[n_].detach().cpu().numpy().copy()
    return out


@pytest.mark.parametrize("mode,pdrop", [("fp32", None), ("bf16", None), ("bf16", 0.1)], ids=["fp32", "bf16", "bf16-dropout0.1"])
def test_dualformer_steps_bit_reproducible(dev, mode, pdrop):
    """the three-step Dualformer run of test_dualformer_train_steps_golden (same config and fixtures) twice, with the dropout rates of
    the config and once more with 0.1 (host-side seeds from Trainer(deterministic=True)): losses, logged scalars, the watched
    gradients and parameters are bit-equal"""
    a, b, moved = _two_runs(lambda: _dualformer_run(dev, mode, pdrop))
    assert moved == 0, f"{moved} unordered launches in a deterministic run"
    _assert_records_equal(a, b)


# ---- the mode off is untouched -------------------------------------------------------------------------------------------------------
def test_mode_off_is_untouched(dev):
    """a convolution and a GroupNorm (small-integer inputs: every partial sum is exact, so the default path's atomics cannot differ
    from run to run either) give the same bits before the mode was switched on and after it was switched off again"""
    from dynamicvectorquantization_amd import kernels as K
    from dynamicvectorquantization_amd import runtime as rt
    from dynamicvectorquantization_amd.layers import Conv2d, Normalize
    torch.manual_seed(4)
    conv, norm = Conv2d(64, 64, 3, 1, 1).to(dev), Normalize(64).to(dev)
    x = torch.randint(-4, 5, (2, 64, 64, 64), device=dev).float()

    def launch():
        with rt.compute_dtype_ctx(torch.bfloat16), torch.no_grad():
            return [conv(x).float(), norm(x).float()]

    assert not K.deterministic()
    before = launch()
    try:
        K.set_deterministic(True)
        launch()
    finally:
        K.set_deterministic(False)
    for a, b in zip(before, launch()):
        assert torch.equal(a, b)
