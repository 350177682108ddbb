"""tests/stage1_norm_math.py against torch in fp64 (no GPU): the references the device tests of test_gpu_groupnorm_kernels.py compare with
are themselves checked against F.group_norm, F.batch_norm (train and eval, with its buffers) and autograd.

Agreement: 1e-12 relative, |a - ref| <= 1e-12 (|ref| + mean|ref|) per element -- the second term because both sides are fp64 sums whose
cancelling elements carry the rounding of the tensor's typical magnitude, not of their own."""
import pytest
import torch
import torch.nn.functional as F

import stage1_norm_math as M

RTOL = 1e-12
ACTS = pytest.mark.parametrize("kind", [M.ACT_NONE, M.ACT_SWISH, M.ACT_LRELU], ids=["none", "swish", "lrelu"])


def _close(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    bound = RTOL * (ref.abs() + ref.abs().mean())
    bad = (a - ref).abs() > bound
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ, worst {float((a - ref).abs().max()):.3e}"


def _torch_act(z, kind):
    if kind == M.ACT_SWISH:
        return F.silu(z)
    if kind == M.ACT_LRELU:
        return F.leaky_relu(z, 0.2)
    return z


def _draw(seed, shape, c):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, c, generator=g, dtype=torch.float64) * 1.5 + 0.7
    dy = torch.randn(*shape, c, generator=g, dtype=torch.float64)
    add = torch.randn(*shape, c, generator=g, dtype=torch.float64)
    gamma = 1 + 0.2 * torch.randn(c, generator=g, dtype=torch.float64)
    beta = 0.2 * torch.randn(c, generator=g, dtype=torch.float64)
    return x, dy, add, gamma, beta


# (N, H, W, C, G): groups of 1, 2, 3, 12 and 64 channels, N = 1 and N > 1
SHAPES = [(2, 5, 7, 8, 8), (3, 4, 4, 64, 32), (2, 5, 13, 96, 32), (2, 3, 11, 96, 8), (1, 7, 10, 128, 2), (2, 1, 1, 128, 32)]


@ACTS
@pytest.mark.parametrize("n,h,w,c,g", SHAPES, ids=[f"{n}x{h}x{w}x{c}-cpg{c // g}" for n, h, w, c, g in SHAPES])
def test_groupnorm(n, h, w, c, g, kind):
    eps = 1e-6
    x, dy, add, gamma, beta = _draw(n + h + c + g, (n, h, w), c)
    y, z, mean, rstd = M.gn_forward(x, gamma, beta, g, eps, kind)
    xt, gt, bt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    zt = F.group_norm(xt.permute(0, 3, 1, 2), g, gt, bt, eps).permute(0, 2, 3, 1)
    yt = _torch_act(zt, kind)
    _close(y, yt)
    _close(z, zt)
    v = x.reshape(n, h * w, g, c // g)
    _close(mean, v.mean(dim=(1, 3)))
    _close(rstd, 1.0 / torch.sqrt(v.var(dim=(1, 3), unbiased=False) + eps))
    s, q, a = M.group_sums(x, g)
    _close(s, v.sum(dim=(1, 3)))
    _close(q, (v * v).sum(dim=(1, 3)))
    _close(a, v.abs().sum(dim=(1, 3)))
    # the {scale, shift} table applies the same affine map
    ss = M.scale_shift(mean, rstd, gamma, beta)
    _close(x * ss[:, None, None, :, 0] + ss[:, None, None, :, 1], zt)
    # backward, without and with the gradient of a residual branch
    (yt * dy).sum().backward()
    dx, dg, db = M.gn_backward(x, dy, gamma, beta, g, kind, mean, rstd)
    _close(dx, xt.grad)
    _close(dg, gt.grad)
    _close(db, bt.grad)
    dxa, dga, dba = M.gn_backward(x, dy, gamma, beta, g, kind, mean, rstd, addend=add)
    xt.grad = None
    zt2 = F.group_norm(xt.permute(0, 3, 1, 2), g, gt, bt, eps).permute(0, 2, 3, 1)
    ((_torch_act(zt2, kind) * dy).sum() + (xt * add).sum()).backward()
    _close(dxa, xt.grad)
    assert torch.equal(dga, dg) and torch.equal(dba, db)


@ACTS
@pytest.mark.parametrize("c", [8, 16, 24])
def test_fixed_statistics_backward(c, kind):
    """constant statistics: y = act((x - mean) rstd gamma + beta) is a per-channel affine map; autograd of that map"""
    x, dy, add, gamma, beta = _draw(c, (2, 3, 5), c)
    g = torch.Generator().manual_seed(100 + c)
    mean = torch.randn(1, c, generator=g, dtype=torch.float64)
    rstd = 0.5 + torch.rand(1, c, generator=g, dtype=torch.float64)
    flat, dflat = x.reshape(1, -1, c), dy.reshape(1, -1, c)
    xt, gt, bt = flat.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yt = _torch_act((xt - mean[0]) * rstd[0] * gt + bt, kind)
    y, _, _, _ = M.gn_forward(flat, gamma, beta, c, 0.0, kind, mean=mean, rstd=rstd)
    _close(y, yt)
    (yt * dflat).sum().backward()
    dx, dg, db = M.gn_backward(flat, dflat, gamma, beta, c, kind, mean, rstd, fixed_stats=True)
    _close(dx, xt.grad)
    _close(dg, gt.grad)
    _close(db, bt.grad)
    dxa, _, _ = M.gn_backward(flat, dflat, gamma, beta, c, kind, mean, rstd, addend=add.reshape(1, -1, c), fixed_stats=True)
    _close(dxa, xt.grad + add.reshape(1, -1, c))


@ACTS
@pytest.mark.parametrize("n,h,w,c", [(2, 9, 7, 16), (1, 2, 3, 8), (3, 4, 5, 24)])
def test_batchnorm(n, h, w, c, kind):
    eps, momentum = 1e-5, 0.1
    x, dy, _, gamma, beta = _draw(n * h + c, (n, h, w), c)
    g = torch.Generator().manual_seed(c)
    rm0 = torch.randn(c, generator=g, dtype=torch.float64)
    rv0 = 0.5 + torch.rand(c, generator=g, dtype=torch.float64)
    xt, gt, bt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    zt = F.batch_norm(xt.permute(0, 3, 1, 2), rm, rv, gt, bt, True, momentum, eps).permute(0, 2, 3, 1)
    yt = _torch_act(zt, kind)
    _close(M.bn_train(x, gamma, beta, eps, kind), yt)
    rm_ref, rv_ref = M.bn_running_update(x, rm0, rv0, momentum)
    _close(rm_ref, rm)
    _close(rv_ref, rv)
    # backward: GroupNorm with one group per channel over [1, N H W, C]
    (yt * dy).sum().backward()
    mean, var = M.bn_batch_stats(x)
    dx, dg, db = M.gn_backward(x.reshape(1, -1, c), dy.reshape(1, -1, c), gamma, beta, c, kind, mean[None], M.rstd_of(var, eps)[None])
    _close(dx.reshape(x.shape), xt.grad)
    _close(dg, gt.grad)
    _close(db, bt.grad)
    # eval mode: the running statistics
    ze = F.batch_norm(x.permute(0, 3, 1, 2), rm, rv, gamma, beta, False, momentum, eps).permute(0, 2, 3, 1)
    _close(M.bn_eval(x, rm, rv, gamma, beta, eps, kind), _torch_act(ze, kind))
    # the same through given statistics: {sum, sum of squares} = count {mean, var + mean^2}
    y2, _, _, _ = M.gn_forward(x.reshape(1, -1, c), gamma, beta, c, eps, kind, mean=rm[None], rstd=M.rstd_of(rv, eps)[None])
    _close(y2.reshape(x.shape), _torch_act(ze, kind))


@ACTS
def test_actnorm(kind):
    """h = scale (x + loc), and the statistics the layer hands to the kernels (mean = -loc, var = 1 - eps: rstd = 1) give the same"""
    c, eps = 16, 1e-5
    x, dy, _, scale, loc = _draw(7, (2, 9, 7), c)
    xt, st, lt = x.clone().requires_grad_(True), scale.clone().requires_grad_(True), loc.clone().requires_grad_(True)
    yt = _torch_act(st * (xt + lt), kind)
    _close(M.actnorm_forward(x, loc.reshape(1, c, 1, 1), scale.reshape(1, c, 1, 1), kind), yt)
    mean, rstd = (-loc)[None], M.rstd_of(torch.full((1, c), 1.0 - eps, dtype=torch.float64), eps)
    _close(rstd, torch.ones(1, c, dtype=torch.float64))
    flat = x.reshape(1, -1, c)
    y2, _, _, _ = M.gn_forward(flat, scale, torch.zeros(c), c, eps, kind, mean=mean, rstd=rstd)
    _close(y2.reshape(x.shape), yt)
    (yt * dy).sum().backward()
    dx, dscale, dsum = M.gn_backward(flat, dy.reshape(1, -1, c), scale, torch.zeros(c), c, kind, mean, rstd, fixed_stats=True)
    _close(dx.reshape(x.shape), xt.grad)
    _close(dscale, st.grad)                      # d scale = sum dz (x + loc)
    _close(dsum * scale, lt.grad)                # d loc = scale sum dz


def test_bf16_round():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, -3.0e-5, 0.1], dtype=torch.float32)
    r = M.bf16_round(x)
    assert r.dtype == torch.float32 and torch.equal(r, x.to(torch.bfloat16).float())
    assert float(r[1]) == 1.0 and float(r[2]) == 1.015625          # ties to even: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 4 2^-8
